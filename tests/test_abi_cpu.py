"""The C ABI without a GPU: every surface registered in _lib.SURFACES against its public header -- prototypes, the loaded handle,
struct mirrors, constants -- and the registry as a whole against include/.  With ctypes a parameter, a field or an array length that
differs on one side only is silent garbage on the stack; here it is a CPU-suite failure, for every surface by the same check."""
import ctypes
import importlib
import os

import pytest

import abi_check as A

L = importlib.import_module("3danimals_amd._lib")
COUNTS = {"a3d.h": 91, "a3d_bsdf.h": 5, "a3d_deriv.h": 4, "a3d_tangent.h": 5, "a3d_reg.h": 8, "a3d_envshade.h": 2, "a3d_sdfreg.h": 2,
          "a3d_edt.h": 2, "a3d_fields.h": 3, "a3d_eval.h": 4}
surfaces = pytest.mark.parametrize("surface", L.SURFACES, ids=[s.header for s in L.SURFACES])


def field_mismatches(mirror, header):
    """What differs between two [(name, ctypes type)] lists: names and order, the ctypes type, the array length."""
    def shape(t):
        return (t._type_, t._length_) if issubclass(t, ctypes.Array) else (t, None)

    if [n for n, _ in mirror] != [n for n, _ in header]:
        return [("names", [n for n, _ in mirror], [n for n, _ in header])]
    return [(n, shape(a), shape(b)) for (n, a), (_, b) in zip(mirror, header) if shape(a) != shape(b)]


@surfaces
def test_prototypes_match_the_signature_table(surface):
    protos = A.prototypes(surface.header)
    assert set(protos) == set(surface.signatures), set(protos) ^ set(surface.signatures)
    assert not any(k.startswith("?") for ret, params in protos.values() for k in [ret] + params), "unparsed parameter kind"
    bad = [(name, "header", protos[name], "ctypes", A.kinds(sig)) for name, sig in surface.signatures.items() if protos[name] != A.kinds(sig)]
    assert not bad, bad


@surfaces
def test_loaded_library_exports_and_binds_every_entry_point(surface):
    """lib() loops over the merged table: what it set on the handle is this surface's table, symbol by symbol."""
    lib = L.lib()  # loads without a GPU (links libamdhip64 only)
    for name, (res, args) in surface.signatures.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert L.SIGNATURES[name] == (res, args), name


@surfaces
def test_struct_mirrors_match_the_header_field_for_field(surface):
    assert A.struct_names(surface.header) == list(surface.structs), (A.struct_names(surface.header), list(surface.structs))
    for name, mirror in surface.structs.items():
        want = A.struct_fields(name)
        assert not field_mismatches(mirror._fields_, want), (name, field_mismatches(mirror._fields_, want))
        assert mirror._fields_[0] == ("size", ctypes.c_uint32), name
        assert sum(mirror is m for s in L.SURFACES for m in s.structs.values()) == 1, name


@surfaces
def test_registered_constants_equal_their_defines(surface):
    macros = A.defines(surface.header)
    for macro, value in surface.constants.items():
        assert macros.get(macro) == value, (macro, macros.get(macro), value)


def test_registry_is_exactly_the_headers_of_include():
    assert sorted(s.header for s in L.SURFACES) == sorted(os.listdir(A.INCLUDE))
    assert {s.header: len(s.signatures) for s in L.SURFACES} == COUNTS and list(COUNTS) == [s.header for s in L.SURFACES]
    assert len(L.SIGNATURES) == sum(COUNTS.values()) == 126
    for i, a in enumerate(L.SURFACES):
        for b in L.SURFACES[i + 1:]:
            assert not set(a.signatures) & set(b.signatures), (a.header, b.header)
            assert not set(a.structs) & set(b.structs) and not set(a.constants) & set(b.constants), (a.header, b.header)
    assert set(L.SIGNATURES) == {name for s in L.SURFACES for name in s.signatures}
    assert sum(len(s.structs) for s in L.SURFACES) == 13
    mirrors = [c for c in vars(L).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert sorted(m.__name__ for m in mirrors) == sorted(m.__name__ for s in L.SURFACES for m in s.structs.values())  # none unregistered
    assert L.lib().a3d_version() == L.ABI_VERSION == 405


def test_the_checks_bite():
    """An extra int on one side only, an int where the header has a pointer, a float array one element short: each is reported."""
    protos = A.prototypes("a3d.h")
    res, args = L.SIGNATURES["a3d_rast_fwd"]
    assert protos["a3d_rast_fwd"] == A.kinds((res, args)) != A.kinds((res, args + [ctypes.c_int]))
    assert protos["a3d_rast_fwd"][1][:2] == ["ptr", "int"]
    assert sum(len(params) for _, params in protos.values()) > 400
    bsdf = A.prototypes("a3d_bsdf.h")
    assert bsdf["a3d_bsdf_fwd"] != ("int", ["ptr"]) and bsdf["a3d_bsdf_rows"][0] == "int64"
    assert A.prototypes("a3d_edt.h")["a3d_edt_fwd"][1][7] == "double"
    want = A.struct_fields("a3d_estimate_bones_args")
    assert dict(want)["ramp"]._length_ == 9 and dict(want)["attach"]._type_ is ctypes.c_int32 and len(want) == 16
    short = [(n, ctypes.c_float * 8 if n == "ramp" else t) for n, t in L.EstimateBonesArgs._fields_]
    assert field_mismatches(short, want) == [("ramp", (ctypes.c_float, 8), (ctypes.c_float, 9))]
    as_int = [(n, ctypes.c_int32 * 9 if n == "ramp" else t) for n, t in L.EstimateBonesArgs._fields_]
    assert field_mismatches(as_int, want) == [("ramp", (ctypes.c_int32, 9), (ctypes.c_float, 9))]
    assert field_mismatches(L.EstimateBonesArgs._fields_[:-1], want)[0][0] == "names"
    assert dict(A.struct_fields("a3d_env_shade_desc"))["spec"]._length_ == A.defines("a3d.h")["A3D_TEX_MAX_LEVELS"] == 16  # a macro of another header
