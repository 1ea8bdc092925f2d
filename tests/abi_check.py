"""The headers read as data -- the public ones (include/*.h) and the internal ones of _lib.INTERNAL_SURFACES (3danimals_amd/csrc/) --
for the tests that hold 3danimals_amd/_lib.py to them: the a3d_* prototypes by parameter kind, the typedef'd structs as ctypes fields,
the integer #defines.  tests/test_abi_cpu.py checks every registered surface with these; the feature tests use them for their own
spot-checks.  A header is given as its Surface, or as a file name under include/.  (Small regular-expression readers of THESE headers'
style -- one declaration per ';', no function pointers, no nested structs -- not a C parser.)"""
import ctypes
import importlib
import os
import re

INTERNAL_SURFACES = importlib.import_module("3danimals_amd._lib").INTERNAL_SURFACES
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# ctypes type -> the kind a prototype parameter of that type parses to
KIND = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_int64: "int64", ctypes.c_float: "float", ctypes.c_double: "double",
        ctypes.c_size_t: "size_t", ctypes.c_char_p: "char_p"}
_SCALARS = {"int": "int", "int32_t": "int", "int64_t": "int64", "float": "float", "double": "double", "size_t": "size_t"}
_FIELD_TYPES = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
                "double": ctypes.c_double}


def kinds(signature):
    """A (restype, argtypes) entry of a signature table in the vocabulary of prototypes()."""
    res, args = signature
    return KIND[res], [KIND[a] for a in args]


def _code(header):
    """The header's text without comments (a Surface knows its own path; a name alone is looked up under include/)."""
    text = open(getattr(header, "path", None) or os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _kind(decl):
    decl = decl.strip()
    if "*" in decl or re.search(r"\ba3d_stream_t\b", decl):
        return "char_p" if re.match(r"const\s+char\s*\*$", decl) else "ptr"
    base = re.sub(r"\b(const|unsigned)\b", "", decl).split()
    return _SCALARS.get(base[0] if base else "", "?" + decl)  # "?...": a type this reader does not know (the ABI test refuses it)


def prototypes(header):
    """name -> (return kind, [parameter kinds]) of every a3d_* prototype; kinds: ptr, char_p, int, int64, float, double, size_t."""
    code = re.sub(r"^\s*#[^\n]*", "", _code(header), flags=re.M)
    code = re.sub(r"typedef struct.*?\}\s*\w+;", "", code, flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_\s\*]*?)\b(a3d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code):
        ret, name, params = re.sub(r"\b(A3D_API|extern|\"C\")\b", "", m.group(1)), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        # (a parameter's own name goes, unless the declaration ends in '*' and has none)
        protos[name] = (_kind(ret), [_kind(p if p.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*\s*$", "", p)) for p in plist])
    return protos


def defines(header):
    """macro -> value of the header's integer #defines (`#define A3D_X 5`, `#define A3D_Y (-1)`)."""
    return {k: int(v) for k, v in re.findall(r"^[ \t]*#define[ \t]+(A3D_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", _code(header), flags=re.M)}


def struct_names(header):
    """The typedef'd structs of one header, in its order."""
    return re.findall(r"typedef struct (\w+) \{.*?\} \1;", _code(header), flags=re.S)


def struct_fields(struct_name):
    """[(field, ctypes type)] of a typedef'd struct of any header, public or internal, as a ctypes mirror must list them: pointers are
    c_void_p, `name[N]` and `name[A3D_MACRO]` are arrays (the macro is one of include/, maybe of another header: a3d_envshade.h sizes
    with a3d.h's A3D_TEX_MAX_LEVELS), `int32_t a, b;` is two fields."""
    headers = sorted(os.listdir(INCLUDE))
    macros = {k: v for h in headers for k, v in defines(h).items()}
    typedef = r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name)
    bodies = [b for h in headers + list(INTERNAL_SURFACES) for b in re.findall(typedef, _code(h), flags=re.S)]
    assert len(bodies) == 1, (struct_name, len(bodies))
    fields = []
    for decl in (re.sub(r"\s+", " ", d.strip()) for d in bodies[0].split(";") if d.strip()):
        m = re.match(r"(?:const )?(\w+) ?(.*)$", decl)
        for item in (v.strip() for v in m.group(2).split(",")):
            star, name, n = re.match(r"(\*?) ?(\w+)(?:\[(\w+)\])?$", item).groups()
            base = ctypes.c_void_p if star else _FIELD_TYPES[m.group(1)]
            fields.append((name, base * (int(n) if n.isdigit() else macros[n]) if n else base))
    return fields
