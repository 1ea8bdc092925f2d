"""The C ABI without a GPU: every surface registered in _lib.SURFACES (the public headers of include/) and _lib.INTERNAL_SURFACES (the
internal headers of csrc/) against its header -- prototypes, the loaded handle, struct mirrors, constants -- and the registry as a whole
against include/ and against the entry points the sources define.  With ctypes a parameter, a field or an array length that differs on
one side only is silent garbage on the stack; here it is a CPU-suite failure, for every surface by the same check."""
import ctypes
import glob
import importlib
import os
import re

import pytest

import abi_check as A

L = importlib.import_module("3danimals_amd._lib")
COUNTS = {"a3d.h": 91, "a3d_bsdf.h": 5, "a3d_deriv.h": 4, "a3d_tangent.h": 5, "a3d_reg.h": 8, "a3d_envshade.h": 2, "a3d_sdfreg.h": 2,
          "a3d_edt.h": 2, "a3d_fields.h": 3, "a3d_eval.h": 4}
INTERNAL_COUNTS = {"fieldgrad.h": 7, "articulation.h": 4, "pose.h": 5, "eb_common.h": 0}
PUBLIC_ENTRY_POINTS, BOUND_ENTRY_POINTS, VERSION, PUBLIC_STRUCTS, INTERNAL_STRUCTS = 126, 142, 405, 13, 1
surfaces = pytest.mark.parametrize("surface", L.ALL_SURFACES, ids=[s.header for s in L.ALL_SURFACES])


def field_mismatches(mirror, header):
    """What differs between two [(name, ctypes type)] lists: names and order, the ctypes type, the array length."""
    def shape(t):
        return (t._type_, t._length_) if issubclass(t, ctypes.Array) else (t, None)

    if [n for n, _ in mirror] != [n for n, _ in header]:
        return [("names", [n for n, _ in mirror], [n for n, _ in header])]
    return [(n, shape(a), shape(b)) for (n, a), (_, b) in zip(mirror, header) if shape(a) != shape(b)]


@surfaces
def test_prototypes_match_the_signature_table(surface):
    protos = A.prototypes(surface)
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
        assert L.BOUND_SIGNATURES[name] == (res, args), name
        assert (name in L.SIGNATURES) == (not surface.internal), name


@surfaces
def test_struct_mirrors_match_the_header_field_for_field(surface):
    assert A.struct_names(surface) == list(surface.structs), (A.struct_names(surface), list(surface.structs))
    for name, mirror in surface.structs.items():
        want = A.struct_fields(name)
        assert not field_mismatches(mirror._fields_, want), (name, field_mismatches(mirror._fields_, want))
        assert surface.internal or mirror._fields_[0] == ("size", ctypes.c_uint32), name  # (a public struct says its own size)
        assert sum(mirror is m for s in L.ALL_SURFACES for m in s.structs.values()) == 1, name


@surfaces
def test_registered_constants_equal_their_defines(surface):
    macros = A.defines(surface)
    for macro, value in surface.constants.items():
        assert macros.get(macro) == value, (macro, macros.get(macro), value)
    if surface.internal:  # an internal header has no macro this module does not mirror
        assert set(macros) == set(surface.constants), set(macros) ^ set(surface.constants)


def test_registry_is_exactly_the_headers_of_include():
    assert sorted(s.header for s in L.SURFACES) == sorted(os.listdir(A.INCLUDE))
    assert not any(s.internal for s in L.SURFACES) and all(os.path.dirname(s.path) == A.INCLUDE for s in L.SURFACES)
    assert {s.header: len(s.signatures) for s in L.SURFACES} == COUNTS and list(COUNTS) == [s.header for s in L.SURFACES]
    assert len(L.SIGNATURES) == sum(COUNTS.values()) == PUBLIC_ENTRY_POINTS
    assert set(L.SIGNATURES) == {name for s in L.SURFACES for name in s.signatures}
    assert sum(len(s.structs) for s in L.SURFACES) == PUBLIC_STRUCTS
    assert L.lib().a3d_version() == L.ABI_VERSION == VERSION


def test_whole_registry_is_exactly_the_entry_points_the_sources_define():
    """Public and internal surfaces together: disjoint, every ctypes mirror registered, and the bound table is the set of extern "C"
    a3d_* definitions of csrc/*.hip -- an internal entry point has no header under include/, and one defined but registered nowhere
    is found here.  (The profiling setters come from a macro of a3d_common.h and are not entry points of any header.)"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc")
    assert all(s.internal and os.path.dirname(s.path) == csrc for s in L.INTERNAL_SURFACES) and L.ALL_SURFACES == L.SURFACES + L.INTERNAL_SURFACES
    assert {s.header: len(s.signatures) for s in L.INTERNAL_SURFACES} == INTERNAL_COUNTS
    assert sum(len(s.structs) for s in L.INTERNAL_SURFACES) == INTERNAL_STRUCTS
    for i, a in enumerate(L.ALL_SURFACES):
        for b in L.ALL_SURFACES[i + 1:]:
            assert not set(a.signatures) & set(b.signatures), (a.header, b.header)
            assert not set(a.structs) & set(b.structs) and not set(a.constants) & set(b.constants), (a.header, b.header)
    assert len(L.BOUND_SIGNATURES) == PUBLIC_ENTRY_POINTS + sum(INTERNAL_COUNTS.values()) == BOUND_ENTRY_POINTS
    assert set(L.BOUND_SIGNATURES) == {name for s in L.ALL_SURFACES for name in s.signatures}
    mirrors = [c for c in vars(L).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert sorted(m.__name__ for m in mirrors) == sorted(m.__name__ for s in L.ALL_SURFACES for m in s.structs.values())  # none unregistered
    defined = [name for path in sorted(glob.glob(os.path.join(csrc, "*.hip")))
               for name in re.findall(r'^extern "C" [\w \*]*\b(a3d_[a-z0-9_]+)\(', open(path).read(), flags=re.M)]
    assert len(defined) == len(set(defined)) and set(defined) == set(L.BOUND_SIGNATURES), set(defined) ^ set(L.BOUND_SIGNATURES)


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
    pose = {s.header: s for s in L.INTERNAL_SURFACES}["pose.h"]  # an internal surface, read from csrc/
    res, args = pose.signatures["a3d_random_view_cameras"]
    assert A.prototypes(pose)["a3d_random_view_cameras"] == A.kinds((res, args)) != A.kinds((res, args + [ctypes.c_int]))
    assert A.prototypes(pose)["a3d_random_view_cameras"][1][:4] == ["ptr", "ptr", "int", "float"]
    want = A.struct_fields("a3d_estimate_bones_args")
    assert dict(want)["ramp"]._length_ == 9 and dict(want)["attach"]._type_ is ctypes.c_int32 and len(want) == 16
    short = [(n, ctypes.c_float * 8 if n == "ramp" else t) for n, t in L.EstimateBonesArgs._fields_]
    assert field_mismatches(short, want) == [("ramp", (ctypes.c_float, 8), (ctypes.c_float, 9))]
    as_int = [(n, ctypes.c_int32 * 9 if n == "ramp" else t) for n, t in L.EstimateBonesArgs._fields_]
    assert field_mismatches(as_int, want) == [("ramp", (ctypes.c_int32, 9), (ctypes.c_float, 9))]
    assert field_mismatches(L.EstimateBonesArgs._fields_[:-1], want)[0][0] == "names"
    assert dict(A.struct_fields("a3d_env_shade_desc"))["spec"]._length_ == A.defines("a3d.h")["A3D_TEX_MAX_LEVELS"] == 16  # a macro of another header
