"""The wide path of a3d_estimate_bones (csrc/bones_wide.hip) without a GPU: what the entry point refuses before it launches, the
workspace rule of the header against its Python mirror, the torch restatement against the golden the GPU test compares the kernels
with, and the inputs the GPU tests construct -- none of them may sit on a rounding edge of the torch statements themselves."""
import ctypes
import importlib
import re

import numpy as np
import pytest
import torch

import abi_check as A
import bones_wide_cases as C
from conftest import golden

L = importlib.import_module("3danimals_amd._lib")
sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
ops = importlib.import_module("3danimals_amd.ops")
A3D_EINVAL = A.defines("a3d.h")["A3D_EINVAL"]


def test_torch_restatement_matches_the_reference_golden():
    g = golden("bones_wide.npz")
    B, F = (int(v) for v in g["shape"])
    seq = C.base(B, F)
    assert int(g["noise_seed"]) == 9 and seq.shape[2] == int(g["V"])
    for tag, thr in (("default", None), ("fauna", 0.4)):
        bones, chain, aux = sk.estimate_bones(seq.clone(), n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=thr, **C.KW)
        np.testing.assert_allclose(bones.numpy(), g[f"{tag}_bones"], atol=1e-6)
        assert repr(chain) == str(g[f"{tag}_chain"]) and [l["body_bone_idx"] for l in aux["legs"]] == list(g[f"{tag}_leg_body_idx"])


def test_workspace_macros_equal_their_mirrors():
    macros = A.defines("a3d.h")
    mirrored = {k: v for k, v in L.SURFACES[0].constants.items() if k.startswith("A3D_EB_")}
    assert len(mirrored) == 7 and all(macros[k] == v for k, v in mirrored.items()), (mirrored, macros)
    # the closed form itself, read out of the header: A3D_EB_WIDE_WORKSPACE_WORDS(N, V) evaluated with the header's numbers
    text = open(A.INCLUDE + "/a3d.h").read()
    body = re.search(r"#define A3D_EB_WIDE_WORKSPACE_WORDS\(N, V\) (.*)", text).group(1).replace("(size_t)", "").replace("/", "//")
    for N, V in [(33, 1), (33, 386), (200, 5720), (1, (1 << 22) + 1), (40, 1024), (40, 1025), (1 << 24, 1)]:
        assert eval(body, dict(macros, N=N, V=V)) == L.eb_wide_workspace_words(N, V), (N, V)
    assert L.eb_wide_workspace_words(33, 1) > 3 * 33 * 1  # small V: more than the one work-group's 3 N V floats
    assert not ops.estimate_bones_is_wide(32, 386) and ops.estimate_bones_is_wide(33, 1) and ops.estimate_bones_is_wide(1, (1 << 22) + 1)


def _args(N, V, workspace=0x1000, **kw):
    """Arguments that never reach a kernel: the pointers are made-up addresses (the calls below are all refused by the validation)."""
    a = L.EstimateBonesArgs(size=ctypes.sizeof(L.EstimateBonesArgs), N=N, pos=0x1000, bones=0x1000, nearest=0x1000, ok=0x1000, V=V,
                            workspace=workspace, n_body=8, n_leg=3, body_mode_y_plus=1, use_y_threshold=0, y_threshold=0.0)
    for i in range(4):
        a.attach[i] = -1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("what,args", [
    ("wide call, null workspace", dict(N=33, V=386, workspace=None)),
    ("wide call, workspace not 16-byte aligned", dict(N=33, V=386, workspace=0x1004)),
    ("more points than torch.quantile takes", dict(N=1 << 12, V=(1 << 12) + 1)),
    ("more points than torch.quantile takes, few instances", dict(N=2, V=(1 << 23) + 1)),
    ("short size", dict(N=33, V=386, size=ctypes.sizeof(L.EstimateBonesArgs) - 8)),
    ("wide call, odd n_body", dict(N=33, V=386, n_body=7)),
    ("wide call, attachment joint out of range", dict(N=200, V=5720, attach_0=8)),
    ("one work-group, null workspace", dict(N=1, V=386, workspace=None)),
    ("one work-group, odd n_body", dict(N=32, V=386, n_body=7)),
    ("one work-group, too many leg bones", dict(N=6, V=386, n_leg=9)),
    ("one work-group, no vertices", dict(N=6, V=0)),
    ("one work-group, short size", dict(N=1, V=386, size=8)),
])
def test_entry_point_refuses_before_any_launch(what, args):
    attach_0 = args.pop("attach_0", None)
    a = _args(**args)
    if attach_0 is not None:
        a.attach[0] = attach_0
    assert L.lib().a3d_estimate_bones(ctypes.addressof(a), None) == A3D_EINVAL, what
    assert b"a3d_estimate_bones: invalid argument" in L.lib().a3d_last_error(), what


def _max_diff(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("name,seq,mode,thr,n_leg,permutable", C.new_inputs(), ids=lambda v: None if isinstance(v, torch.Tensor) else str(v))
def test_constructed_inputs_sit_on_no_rounding_edge(name, seq, mode, thr, n_leg, permutable):
    """The torch restatement in float32 against itself on permuted vertices (another summation order) and in float64: within half of the
    1e-6 the GPU tests allow the kernels, with every quadrant populated -- the other half is the kernels' own."""
    kw = dict(n_leg_bones=n_leg, body_bones_mode=mode, bone_y_threshold=thr, **C.KW)
    bones, chain, _ = sk.estimate_bones(seq.clone(), **kw)  # (raises on an empty quadrant)
    b64, chain64, _ = sk.estimate_bones(seq.double(), **kw)
    assert repr(chain) == repr(chain64) and _max_diff(bones, b64) <= 5e-7, _max_diff(bones, b64)
    if permutable:
        perm = torch.randperm(seq.shape[2], generator=torch.Generator().manual_seed(3))
        bp, chain_p, _ = sk.estimate_bones(seq[:, :, perm].clone(), **kw)
        assert repr(chain) == repr(chain_p) and _max_diff(bones, bp) <= 5e-7, _max_diff(bones, bp)
