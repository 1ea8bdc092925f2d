"""The background's gradient in the fused compositor, without a GPU: the ctypes mirror of a3d_ca_buffer (unchanged), the entry point's
refusal, and what
render._plan_route does with a background that requires grad under the switch FUSED_BACKGROUND_GRAD (off: the routes of every call are
what they were; on: the spp 1 calls go to the fused compositor, the supersampled, the layered and the mask-shaped ones stay where they
are).  The planner's arguments and its patched device helper are those of tests/test_render_route_cpu.py."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import test_render_route_cpu as T  # noqa: E402

L = importlib.import_module("3danimals_amd._lib")
R = T.R


def test_the_gradient_rides_in_a_field_the_struct_already_has():
    """No field, struct or export is added for the background's gradient: the registered mirror of a3d_ca_buffer is field for field the
    header's, ends at g_null with the 112 bytes tests/test_msaa_cpu.py holds it to, and the version stays.  (An appended field, which the
    proposal asked for, cannot coexist with that pin and with tests/test_abi_cpu.py's one-mirror rule: at spp 1, where no null row
    exists, g_null carries the pointer.)"""
    mirror = next(s.structs["a3d_ca_buffer"] for s in L.SURFACES if "a3d_ca_buffer" in s.structs)
    assert mirror is L.CaBuffer
    header = A.struct_fields("a3d_ca_buffer")
    assert [n for n, _ in mirror._fields_] == [n for n, _ in header] and mirror._fields_[-1] == ("g_null", ctypes.c_void_p)
    assert ctypes.sizeof(mirror) == 112 and mirror.g_null.offset == 104
    assert mirror(size=ctypes.sizeof(mirror)).g_null is None  # (NULL unless a caller sets it: no background gradient)
    assert L.ABI_VERSION == 405 and len(L.SIGNATURES) == 126


def test_the_switch_is_off_unless_the_environment_sets_it():
    assert R.FUSED_BACKGROUND_GRAD is (os.environ.get("A3D_FUSED_BACKGROUND_GRAD", "0") not in ("0", ""))
    if "A3D_FUSED_BACKGROUND_GRAD" not in os.environ:
        assert R.FUSED_BACKGROUND_GRAD is False


BASE = dict(res=(32, 32), spp=1, msaa=False, layers=1, bg="grad", autocast=False, nrm=True, w2c_grad=False, tng="present", nets=True)
# (what the call is, with the switch ON: 'fused' = the covered-point path with the fused compositor; 'same' = the route it has with the switch off)
MATRIX = [
    (dict(BASE, modes=["shaded"]), "fused"),
    (dict(BASE, modes=["shaded", "dino_pred"]), "fused"),
    (dict(BASE, modes=["shaded", "flow"]), "fused"),
    (dict(BASE, modes=["shaded", "depth"]), "fused"),
    (dict(BASE, modes=["kd", "normal", "geo_normal", "shading"]), "fused"),
    (dict(BASE, modes=["shaded", "dino_pred"], res=(30, 50)), "fused"),  # (two launches for the list; the compositor all the same)
    (dict(BASE, modes=["shaded", "dino_pred"], spp=2, msaa=True), "same"),
    (dict(BASE, modes=["shaded", "dino_pred"], spp=4, msaa=True), "same"),
    (dict(BASE, modes=["shaded", "dino_pred"], spp=2), "same"),
    (dict(BASE, modes=["shaded", "dino_pred"], layers=2), "same"),
    (dict(BASE, modes=["shaded"], nets=False), "same"),  # the mask-shaped call
    (dict(BASE, modes=["shaded", "dino_pred"], bg="plain"), "same"),
    (dict(BASE, modes=["shaded", "dino_pred"], bg="none"), "same"),
    (dict(BASE, modes=["shaded"], nets=False, bg="plain"), "same"),
]


@pytest.fixture
def planner(monkeypatch):
    """tests/test_render_route_cpu.py's: the device helper says yes, autocast is a flag, every switch is restored afterwards -- the
    background switch and FUSED_MSAA (on here, so that the supersampled route exists to stay away from) among them."""
    flag = [False]
    monkeypatch.setattr(R, "_on_gpu_f32", lambda t: torch.is_tensor(t))
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: flag[0])
    for s in T.SWITCHES:
        monkeypatch.setattr(R, s, T.ON[s])
    monkeypatch.setattr(R, "FUSED_BACKGROUND_GRAD", False)
    return flag


@pytest.mark.parametrize("args,want", MATRIX, ids=[f"{'+'.join(a['modes'])}-{a['res'][0]}x{a['res'][1]}-spp{a['spp']}{'m' if a['msaa'] else ''}-L{a['layers']}-"
                                                   f"{a['bg']}{'' if a['nets'] else '-nonets'}" for a, _ in MATRIX])
def test_routes_with_the_switch_off_and_on(args, want, planner, monkeypatch):
    off = T.plan(args, planner)
    T.check_invariants(off, args, dict(T.ON))  # (the existing file's invariants: with the switch off they hold as they are)
    if args["bg"] == "grad":  # today's routes: no fused compositor behind a background that requires grad
        assert not off.composite and off.path in ("covered", "dense", "layers"), off
        if args["layers"] == 1 and (args["spp"] > 1 or "depth" in args["modes"]):
            assert off.path == "dense", off
    monkeypatch.setattr(R, "FUSED_BACKGROUND_GRAD", True)
    on = T.plan(args, planner)
    if want == "same":
        assert on == off, (on, off)
        if args["spp"] > 1:
            assert on.path == "dense", on  # (neither the supersampled route nor a point list)
        return
    assert on.path == "covered" and on.composite and args["spp"] == 1, on
    assert on.one_launch == (args["res"][0] % 8 == 0 and args["res"][1] % 8 == 0) and on.defer == on.one_launch, on
    assert on.served == frozenset(args["modes"]) & {"depth", "tangent"}, on
    plain = T.plan(dict(args, bg="plain"), planner)
    assert on == plain, (on, plain)  # the route of the same call with a background that does not require grad


def test_the_switch_moves_nothing_without_a_background_that_requires_grad(planner, monkeypatch):
    """Every argument combination of tests/test_render_route_cpu.py's small set, under all switches on: the same record with the switch on
    and off unless the background requires grad, and then only towards the fused compositor at spp 1."""
    moved = 0
    for a in T.arg_sets(full=False):
        monkeypatch.setattr(R, "FUSED_BACKGROUND_GRAD", False)
        off = T.plan(a, planner)
        monkeypatch.setattr(R, "FUSED_BACKGROUND_GRAD", True)
        on = T.plan(a, planner)
        if a["bg"] != "grad":
            assert on == off, (a, on, off)
        elif on != off:
            moved += 1
            assert a["spp"] == 1 and a["layers"] == 1 and on.path == "covered" and on.composite and not off.composite, (a, on, off)
    assert moved > 0


def test_entry_point_refuses_a_background_gradient_without_a_background():
    """g_null at spp 0 / 1 is the background's gradient: with bg == NULL it is A3D_EINVAL from the argument checks, for either buffer,
    before anything is launched (no GPU here: a launch would be another error).  On a supersampled call the field is the null rows'
    gradient as it always was: the same struct with spp = 2 is not refused for it."""
    lib, fake, full = L.lib(), 0x1000, ctypes.sizeof(L.CaBuffer)
    bwd = lambda b, second=None: lib.a3d_composite_aa_bwd(ctypes.addressof(b), None if second is None else ctypes.addressof(second), fake, 4, fake, fake, fake,
                                                          4096, fake, 1, fake, 1, 3, 1, 8, 8, fake, None, None)
    plain = L.CaBuffer(size=full, C=3, vals=fake, g_out=fake, g_vals=fake)
    asks = lambda **kw: L.CaBuffer(size=full, C=3, vals=fake, g_out=fake, g_vals=fake, g_null=fake, **kw)
    for what, (first, second) in {"first": (asks(), None), "spp = 1": (asks(spp=1), None), "second": (plain, asks())}.items():
        assert bwd(first, second) != 0, what
        err = lib.a3d_last_error().decode()
        assert "invalid argument" in err and err.endswith("invalid argument: b->bg"), (what, err)
    ms = asks(spp=2, aa=1, cover_rast=fake, null_vals=None)  # (refused, but for its missing null rows, not for the gradient pointer)
    assert bwd(ms) != 0 and "ms_check" in lib.a3d_last_error().decode() and "null_vals" in lib.a3d_last_error().decode()
