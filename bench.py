#!/usr/bin/env python
"""Benchmark of the reconstruct-and-render hot path:  python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): train_magicpony_horse-like synthetic step,
batch 16 per GPU @ 256x256, forward + backward + Adam -- DMTet on a Kuhn R=64 grid (the stand-in for the reference's
"128" Quartet grid), instance deformation, skinning with 20 bones, three make_mesh passes, rasterise /
interpolate / antialias, the SDF / texture / DINO / light / deformation MLPs at the reference's sizes, photometric + mask +
DINO-feature losses and the shape regularisers.  See 3danimals_amd/pipeline.py.  `--workload fauna|ponymation` runs the per-rank
steps of configs[3] / configs[4] instead (same JSON contract; `config.workload` says which).

N > 1: launched by the driver through torch.distributed.run, one rank per GPU, DDP over RCCL (gradient all-reduce of
the MLP parameters; the hot-path kernels themselves exchange nothing: images shard over the batch) -> weak scaling.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps, writes the last
step's outputs if `--dump-outputs DIR` is given, and prints the line.  `--full` adds these extra objects (each measured in runs of its
own after the timed steps; `--no-*` switches leave single ones out):
  extra_legs   -- N > 1: every rank on its own poses and the Fauna per-rank step; 1 GPU magicpony: the trained-like (spiky) mesh;
  rank_diagnostics -- N > 1: per-rank blocking synchronisations and GPU-busy time per step;
  roofline     -- the dominant IN-SCOPE entry point of the hot path (DMTet, skinning, normals, topology,
                  rasterise, covered pixels, G-buffer, shading, antialias): algorithmic bytes per launch / mean launch duration measured
                  live with HIP events on the launch stream, against the 8 TB/s HBM peak; `in_scope` = the bytes-weighted aggregate
                  over all of them per step; `with_f3_losses` adds the fused reconstruction losses; `networks_side`
                  = the kernels that serve model/networks (out of scope, reported for completeness);
  parity       -- the step the CPU oracle re-runs for `cpu_baseline` compared with the HIP step it was snapshotted from;
  dropin       -- the same step with the networks evaluated exactly as the reference's model/networks does (--networks reference);
  cpu_baseline -- the CPU oracle (kind "port") timed on this box's host cores on a bounded sample of the batch;
  attribution, box, host_syncs, config1_geometry, kernels -- launch attribution, box fingerprint, blocking synchronisations of one
                  step, BASELINE configs[1] beside the CPU oracle, the per-entry-point event times behind the roofline.

`--dump-outputs DIR`: what the timed path handed its caller in the last timed step (the step's output dict: images, losses, ...) as
DIR/<name>.npy, float32 (float64 stays float64); an array of more than DUMP_SAMPLE elements is stored as a fixed, seeded sample of
them (the same indices in every run of the same arguments), so that two builds can be compared output for output.  The inputs are
seeded, and by default every warm-up and timed step of the headline starts from the scene's initial weights and optimiser state
(from_initial_state), so that two runs of the same arguments differ by rounding only (profiles/r07_dump_reproducibility.json).
`--carry-state` times the training trajectory instead (weights and Adam state carried over, the mesh drifting): what the committed
lines and profiles measure (tools/run_bench_lines.sh, tools/prof_bench.sh, tools/pmc_*.sh); its dumps differ from run to run.
"""
import argparse
import contextlib
import importlib
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_FP32_PEAK_TFLOPS = 157.3  # dense fp32-input MFMA (v_mfma_f32_32x32x2_f32), same guide
PMC_TRAFFIC_GLOB = os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")  # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/pmc_traffic.sh)


def kernel_source_sha16():
    """sha256 over the HIP sources the library is built from (3danimals_amd/csrc/*.hip, *.h, in name order): what a PMC traffic file is
    stamped with (tools/pmc_traffic.py), so that a file taken from other kernels is recognised as stale instead of being quoted."""
    import glob
    import hashlib

    h = hashlib.sha256()
    src = os.path.join(ROOT, "3danimals_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.h"))):
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()[:16]


PMC_WORKLOAD = "magicpony grid64 batch16 256x256 train"  # what tools/pmc_traffic.sh profiles (bench.py's default command)


def workload_signature(args, batch):
    return (f"{args.workload} grid{grid_name(args).replace('kuhn', '')} batch{batch} {args.resolution}x{args.resolution} {'forward' if args.forward_only else 'train'}"
            + ("" if getattr(args, "mesh", "quadruped") == "quadruped" else f" mesh-{args.mesh}") + (" no-render" if getattr(args, "no_render", False) else ""))


def grid_name(args):
    return args.grid if args.grid else f"kuhn{args.grid_res}"


def pmc_traffic(signature=PMC_WORKLOAD):
    """(per-call traffic table or None, note, stale flag): the newest committed PMC file whose stamp equals the current kernel sources --
    for the workload it was taken on only (bytes per call depend on the mesh and the batch)."""
    import glob

    if signature != PMC_WORKLOAD:
        return None, f"the committed PMC passes profile the default workload ({PMC_WORKLOAD}), not this one ({signature})", False

    files = sorted(glob.glob(PMC_TRAFFIC_GLOB), reverse=True)
    if not files:
        return None, "no PMC traffic file under profiles/", False
    sha = kernel_source_sha16()
    for f in files:
        rec = json.load(open(f))
        if rec.get("kernel_source_sha16") == sha:
            return rec["per_call"], ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, committed as " + os.path.relpath(f, ROOT) +
                                     f" (kernel sources {sha})"), False
    return None, (f"stale: no PMC traffic file under profiles/ carries the stamp of the current kernel sources ({sha}); newest is "
                  + os.path.relpath(files[0], ROOT) + " -- re-run tools/pmc_traffic.sh"), True

# what the hot path consists of.  f3 = the fused reconstruction losses ("next" row, built).  Everything else
# (rows_*, harmonic_embed, gemm) serves the texture / DINO / SDF fields = model/networks: out of scope.
IN_SCOPE = ("a3d_dmtet_", "a3d_skin_", "a3d_bone_transforms_", "a3d_normals_", "a3d_mesh_topology", "a3d_rast_", "a3d_interp_", "a3d_cover_",
            "a3d_gbuffer_", "a3d_shade_", "a3d_aa_", "a3d_composite_aa_", "a3d_mask_aa_", "a3d_xfm_", "a3d_flow_delta_", "a3d_estimate_bones")
F3 = ("a3d_recon_losses_",)


def algorithmic_bytes(name, d):
    """Algorithmic HBM bytes of ONE call of a C-ABI entry point (DESIGN.md 'Kernels').

    ``name`` may carry a channel tag, e.g. 'a3d_interp_fwd[C3]'.  Index buffers shared over the batch count once.  B = frames
    rendered per step (images x frames), V / F = surface vertices / faces, P = covered pixels, K = bones.
    """
    B, V, F, HW, Nv, Ne, Nt, K = d["B"], d["V"], d["F"], d["H"] * d["W"], d["Nv"], d["Ne"], d["Nt"], d["K"]
    Bv = int(d.get("skin_v_batch", 1))
    if "[defer]" in name:  # the rasteriser's triangle launch alone: the texels are written (and credited) by a3d_rast_resolve_gbuffer_fwd
        return algorithmic_bytes(name.replace("[defer]", ""), d) - 16 * B * HW
    if "[+shade]" in name:  # the colour computed on the spot: G-buffer row + kd in (60 B per point) instead of the shaded row (12 B)
        return algorithmic_bytes(name.replace("[+shade]", ""), d) + 48 * int(d.get("P", 0))
    if name.endswith("[+analysis]"):  # the silhouette analysis rode in this call's first launch: both passes' bytes
        return algorithmic_bytes(name[:-len("[+analysis]")], d) + algorithmic_bytes("a3d_aa_analyze", d)
    if "+C" in name:  # two buffers in one call of the compositor: [C17+C4] = the sum of the single-buffer figures
        base, tags = name.split("[")[0], name.split("[")[1].rstrip("]").split("+")
        return sum(algorithmic_bytes(f"{base}[{t}]", d) for t in tags)
    Ck = name.split("[C")[1].split("]")[0] if "[C" in name else "0"
    C, Cout = (int(Ck.split(">")[0]), int(Ck.split(">")[1])) if ">" in Ck else (int(Ck), int(Ck))  # [C17>16]: 17 composited channels, 16 materialised
    if name.startswith("a3d_normals_fwd_pair["):  # two vertex arrays in one launch, e.g. [B16+B1]: the index data once, the per-image bytes for all
        Bn = sum(int(t.lstrip("B")) for t in name.split("[")[1].rstrip("]").split("+"))
        return 4 * V + 24 * F + Bn * (36 * F + 24 * V)
    if name.startswith("a3d_rast_fwd[N"):  # the vertex normals of [N<Ba>+<Bb>] images ride in the triangle launch: both passes' bytes
        Bn = sum(int(t) for t in name.split("[N")[1].rstrip("]").split("+"))
        return algorithmic_bytes("a3d_rast_fwd", d) + 4 * V + 24 * F + Bn * (36 * F + 24 * V)
    Bn = int(name.split("[B")[1].split("]")[0]) if "[B" in name else B  # batch tag of the normals calls (prior mesh: 1)
    base = name.split("[")[0]
    P = int(d.get("P", 0))
    Pp = -(-P // 8192) * 8192  # render.POINT_BUCKET
    dm_planes = Ne // 8 + Nt // 2 + Ne // 16  # bit planes + word prefixes, written by the count pass and read by the emit pass
    if d.get("dm_words_read"):
        # culled count pass (word groups): the sdf in, the sign plane out and in, 32 B of group ids per 64-row word in, and the index rows
        # of the words it does read (counted for this step's SDF by the kernel's own rule) -- NOT the 8 B/edge + 16 B/tet it used to stream
        we, nwe, wt, nwt = d["dm_words_read"]
        dm_count = 4 * Nv + 2 * (Nv // 8) + 32 * (nwe + nwt) + 64 * (8 * we + 16 * wt) + dm_planes
    else:
        dm_count = 4 * Nv + 8 * Ne + 16 * Nt + dm_planes  # sdf, both index arrays in; bit planes + word prefixes out
    we, nwe, wt, nwt = d.get("dm_words_read") or (0, Ne // 64, 0, Nt // 64)
    table = {
        "a3d_dmtet_count": dm_count,
        # ordered pass: sdf + rank table in, sign plane out and in, 64 B of group ids per word in, the rows (ranks + source row) of the
        # words that are read, the planes cleared, set bit by bit and read once more for the in-block prefixes
        "a3d_dmtet_count_ordered": 8 * Nv + 2 * (Nv // 8) + 64 * (nwe + nwt) + 64 * (12 * we + 20 * wt) + 2 * dm_planes + Nt // 16,
        "a3d_dmtet_emit_sparse": dm_planes + Nt // 16 + 56 * V + 72 * F + 12 * F + (12 * F + 4 * V) + 4 * Nv,
        # emit: bit planes in; per surface vertex: index pair, 2 sdf, 2 positions in, vertex + edge row out; per face: half a tet2edge row in,
        # 48 bytes of int64 indices out
        "a3d_dmtet_emit": dm_planes + 56 * V + 72 * F + 12 * F + (12 * F + 4 * V) + 4 * Nv,  # (+ the dense SDF gradient it clears for the backward)  # (+ the vertex -> face lists it now writes itself)  # (+ the int32 triangle list of the render kernels)
        "a3d_dmtet_bwd": 12 * V + 4 * V + 8 * V + 8 * V + 24 * V + 8 * V,  # g_verts, edge row, index pair, 2 sdf, 2 positions in; two 4-byte adds out (what the memory side makes of them is traffic, not credit)
        "a3d_skin_fwd": 12 * V + 12 * B * V,
        "a3d_skin_bwd": 12 * B * V + 12 * V + 12 * V + 48 * B * K,
        # chain + skinning in one launch: skin_fwd's bytes + the bones / angles in and the transforms (+ chain products) out
        # (rest vertices in and -- backward -- their gradient out: per image when the instance deformation moved them (Bv = B), else once)
        # (round 5: the chain-product scratch the forward leaves for the backward, B K 8 96 bytes each way, is staging -- not credited)
        "a3d_skin_pose_fwd": 12 * Bv * V + 12 * B * V + B * K * (12 + 48 + 24),
        "a3d_skin_pose_bwd": 12 * B * V + 12 * Bv * V + 12 * Bv * V + 48 * B * K + B * K * (12 + 48 + 12 + 24),
        "a3d_normals_adjacency": 24 * F + 4 * V,  # triangle list in, CSR out
        "a3d_mesh_topology": 12 * F + (4 * V + 12 * F) + 12 * F,  # triangle list in; CSR + opposite-vertex table out
        "a3d_mesh_topology_finalize": 12 * F + 4 * V + (4 * V + 12 * F),  # int32 triangle list + valence counts in; offsets + lists out
        "a3d_normals_fwd": 4 * V + 24 * F + Bn * (36 * F + 24 * V),  # CSR + indices once; per image position gathers, acc + nrm out
        # SURVEY 8d "bwd same order": CSR + indices once; per image the position gathers, the accumulated normal and its incoming gradient per
        # vertex in, the position gradient out.  (round 5: the per-face intermediate of the faces-first form -- 72 F B written and read back --
        # and the per-corner re-reads of per-vertex data are staging, not credited)
        "a3d_normals_bwd": 4 * V + 24 * F + Bn * (36 * F + 24 * V + 12 * V),
        "a3d_rast_fwd": B * (16 * V + 16 * HW) + 12 * F,
        "a3d_rast_bwd": B * (32 * HW + 16 * V),
        "a3d_interp_fwd": B * (16 * HW + 4 * C * HW),
        "a3d_interp_bwd": B * (16 * HW + 4 * C * HW + 16 * HW + 4 * C * V),
        "a3d_gbuffer_fwd": P * (8 + 16 + 48),
        # list + map + rows in one launch: the texels of the 256-pixel blocks that hold a covered pixel in (16 B/pixel; the empty blocks are
        # known from the rasteriser's block counts, 4 B each), list + pixel -> entry map + rows out
        "a3d_cover_gbuffer_fwd": 16 * 256 * int(d.get("cover_blocks", B * HW // 256)) + 4 * (B * HW // 256) + 8 * P + 4 * B * HW + 48 * P,
        # resolve + list + rows in one launch: texels out (16 B/pixel), list + pixel -> entry map + rows out; the 8-byte keys it consumes
        # and re-arms are staging (not credited), the texels are not read back at all
        "a3d_rast_resolve_gbuffer_fwd": 16 * B * HW + 8 * P + 4 * B * HW + 48 * P + 20 * Pp,  # (round 6: + the fields' input rows and image index, 12 + 8 B per padded point)
        "a3d_rast_resolve": 16 * B * HW,
        "a3d_gbuffer_bwd": P * (8 + 16 + 48) + B * V * (36 + 16),
        "a3d_gbuffer_prior_grad": 12 * B * V + 12 * V,
        "a3d_estimate_bones": 12 * V + 24 * K,  # the canonical mesh's vertices in (once: the passes over them hit the cache), the bones out
        "a3d_rows_segsum": 4 * Pp * C + 4 * B * C,  # P here = the padded point list the fields see
        "a3d_rows_add_relu_fwd": 8 * Pp * C,  # y read + written in place; rows[B,C] stay in L2
        "a3d_rows_add_relu_bwd": 12 * Pp * C + 4 * B * C,  # g, y in; g_pre out; per-image sums
        "a3d_gemm_nn_relumask": Pp * 256 * 4 * 3 + 256 * 256 * 4,  # A in, X (mask) in, C out; weight from L2.  Compute bound: see flops below
        "a3d_harmonic_embed_fwd": Pp * (12 + 4 * 64),  # texture field's input stage (n = 10: 64 columns); the DINO field's is 52 wide
        "a3d_harmonic_embed_bwd": Pp * (4 * 64 + 12 + 12),
        "a3d_recon_losses_fwd": B * HW * (16 + 64 + 12 + 64 + 12 + 1),  # shaded, dino(16), image_gt, dino_gt, three masks; 'both' out
        "a3d_recon_losses_bwd": B * HW * (16 + 64 + 12 + 64 + 12 + 1 + 16 + 64),
        "a3d_cover_count": 4 * B * HW,  # the id channel of the raster buffer (only for buffers that did not come out of a3d_rast_fwd)
        "a3d_cover_emit": 4 * B * HW + 8 * P + 4 * B * HW,  # id channel in; list + pixel -> entry map out
        # C = channels of the composited image (values + alpha): point rows in, image out (+ the crossing pixels); backward: image
        # gradient read at the covered pixels, point-row gradient out, vertex gradient out
        "a3d_composite_aa_fwd": 4 * B * HW + 4 * P * max(C - 1, 0) + 4 * Cout * B * HW,
        "a3d_composite_aa_bwd": 8 * P + 8 * P * max(C - 1, 0) + 16 * B * V,
        # texture-less render: raster texels in, image out; backward: the silhouette records' share of the image gradient in, vertex gradient out
        "a3d_mask_aa_fwd": 16 * B * HW + 4 * C * B * HW,
        "a3d_mask_aa_bwd": 32 * B * V,
        "a3d_shade_fwd": P * (48 + 8 + 12 + 12 + 4 + 12),  # G-buffer row, image index, kd in; normal, shading, shaded out (camera/light rows: 1 KB table)
        "a3d_shade_bwd": P * (48 + 8 + 12 + 28 + 48 + 12),  # + the three incoming gradients; G-buffer and kd gradients out
        # the adjoint inside the compositor's backward node: colour gradient, G-buffer row, list entry, kd in; G-buffer gradient and the
        # texture field's 9-column output gradient (padded rows) out
        "a3d_shade_bwd_rows": P * (12 + 48 + 8 + 12 + 48) + 36 * Pp,
        "a3d_xfm_points_fwd": B * V * (12 + 16) + 64 * B,
        "a3d_xfm_points_bwd": B * V * (16 + 12 + 12) + 128 * B,
        # render_mesh's per-vertex motion to the next frame ('flow'): clip positions in (every frame once), the 2-D differences out; backward:
        # their gradient and the clip positions in, the clip gradient out
        "a3d_flow_delta_fwd": B * V * (16 + 8),
        "a3d_flow_delta_bwd": B * V * (8 + 16 + 16),
        "a3d_dmtet_gather_rows": 0,  # (a few thousand rows: latency only; credited nothing)
        "a3d_bone_transforms_fwd": B * K * (12 + 48) + 24 * K,
        "a3d_bone_transforms_bwd": B * K * (12 + 48 + 12) + 24 * K,
        "a3d_aa_topology": 12 * F + 12 * F,
        "a3d_aa_analyze": B * 16 * HW + B * 16 * V,
        "a3d_aa_fwd": B * 8 * C * HW,
        "a3d_aa_bwd": B * 8 * C * HW + B * 16 * V,
    }
    return table.get(base)


def _pixel_boxes(sc):
    """Pixel-box statistics of the mesh a scene rendered last (what the rasteriser's cost follows): mean / max box, share above 64 px."""
    clip, tri = sc.last["points"]["clip"], sc.last["shape"].t_pos_idx[0]
    H, W = sc.resolution
    ndc = clip[..., :2] / clip[..., 3:].clamp(min=1e-6)
    c = ((ndc * 0.5 + 0.5) * torch.tensor([W, H], dtype=torch.float32, device=clip.device))[:, tri]
    ext = c.amax(2) - c.amin(2)
    area = (ext[..., 0].clamp(0, W) + 1) * (ext[..., 1].clamp(0, H) + 1)
    return dict(box_px_mean=round(float(area.mean()), 1), box_px_max=round(float(area.max())), box_px_sum_M=round(float(area.sum()) / 1e6, 2),
                frac_boxes_above_64px=round(float((area > 64).float().mean()), 4))


def _cover_blocks(rast):
    """256-pixel blocks (four 8x8 tiles, tile-row-major: the covered-pixel list's order) of the frame that hold a covered pixel."""
    Bf, H, W = rast.shape[:3]
    if H % 8 or W % 8 or (H * W) % 256:
        return Bf * H * W // 256
    tiles = (rast[..., 3] > 0).reshape(Bf, H // 8, 8, W // 8, 8).any(dim=4).any(dim=2)
    return int(tiles.reshape(Bf, -1, 4).any(dim=-1).sum())


def algorithmic_flops(name, d):
    """Flops of ONE call for the compute-bound entry points (None for the bandwidth-bound ones)."""
    Pp = -(-int(d.get("P", 0)) // 8192) * 8192
    return {"a3d_gemm_nn_relumask": 2 * Pp * 256 * 256}.get(name.split("[")[0])


def _aggregate(kernels, prefixes):
    sel = {k: v for k, v in kernels.items() if k.startswith(prefixes) and v["GBps"] is not None}
    tot_b = sum(v["algorithmic_MB"] * v["launches_per_step"] for v in sel.values()) * 1e6
    tot_t = sum(v["mean_us"] * v["launches_per_step"] for v in sel.values()) * 1e-6
    if tot_t <= 0:
        return None
    # frac = total bytes / total time (every microsecond counts alike: the figure the latency-bound calls pull down); frac_bytes_weighted =
    # the mean of the entry points' own fractions weighted by the bytes they move (what a byte of this path sees on average)
    wfrac = sum(v["algorithmic_MB"] * v["launches_per_step"] * v["GBps"] / HBM_PEAK_GBS for v in sel.values()) * 1e6 / max(tot_b, 1.0)
    return dict(us_per_step=round(tot_t * 1e6, 1), algorithmic_MB_per_step=round(tot_b / 1e6, 1), GBps=round(tot_b / tot_t / 1e9, 1),
                frac=round(tot_b / tot_t / 1e9 / HBM_PEAK_GBS, 4), frac_bytes_weighted=round(wfrac, 4),
                entry_point_calls_per_step=round(sum(v["launches_per_step"] for v in sel.values()), 1))


def kernel_pass(scene, module, L, steps, world, dims_of, train=True):
    """Per-entry-point timing of a few steps under HIP events (same workload, separate from the headline timing)."""
    # with DDP, rank 0 alone re-runs a few steps: that must not enqueue collectives the other ranks never join, hence no_sync()
    with L.KernelTimer() as timer, (module.no_sync() if module is not None else contextlib.nullcontext()):
        for _ in range(steps):
            scene.step(module=module, backward=train, optimizer_step=(train and world == 1))
    dims = dims_of(scene)
    kernels = {}
    for name, (count, mean_ms) in sorted(timer.summary().items()):
        ab = algorithmic_bytes(name, dims)
        kernels[name] = dict(launches_per_step=round(count / steps, 2), mean_us=round(mean_ms * 1e3, 2),
                             algorithmic_MB=None if ab is None else round(ab / 1e6, 3),
                             GBps=None if ab is None else round(ab / (mean_ms * 1e-3) / 1e9, 1))
    return kernels, dims


def roofline_of(kernels, dims, signature=PMC_WORKLOAD):
    scope = {k: v for k, v in kernels.items() if k.startswith(IN_SCOPE) and v["GBps"] is not None}
    dom = max(scope, key=lambda k: scope[k]["mean_us"] * scope[k]["launches_per_step"])  # most time per step among the in-scope entry points
    table, traffic_note, stale = pmc_traffic(signature)
    rec = None if table is None else table.get(dom.split("[")[0])
    traffic = None if rec is None else round(rec["traffic_MB"] * 1e6)
    roof = dict(kernel=dom, bound="hbm", achieved=scope[dom]["GBps"], peak=HBM_PEAK_GBS, unit="GB/s", frac=round(scope[dom]["GBps"] / HBM_PEAK_GBS, 4),
                traffic=traffic, traffic_lower_bound=None if rec is None or "traffic_if_all_reads_were_gathers_MB" not in rec else round(rec["traffic_if_all_reads_were_gathers_MB"] * 1e6),
                traffic_stale=stale, traffic_source=traffic_note, launch_us=scope[dom]["mean_us"], launches_per_step=scope[dom]["launches_per_step"],
                algorithmic_bytes_per_launch=round(scope[dom]["algorithmic_MB"] * 1e6), in_scope=_aggregate(kernels, IN_SCOPE),
                with_f3_losses=_aggregate(kernels, IN_SCOPE + F3), mesh=dims)
    # the best-fed streaming kernel of the path, for the other end of the picture
    top = max(scope, key=lambda k: scope[k]["GBps"])
    roof["in_scope_note"] = ("us_per_step is the figure comparable across rounds (round 1: 645.0): fused entry points (compositor, per-image shading rows, "
                             "bit-plane DMTet emit, culled DMTet count) are credited only the bytes they still move, so algorithmic_MB_per_step fell "
                             "with the time")
    cnt = next((k for k in ("a3d_dmtet_count", "a3d_dmtet_count_ordered") if k in scope), None)
    if dims.get("dm_words_read") and cnt:
        # the culled count pass no longer streams the index arrays: its credit fell ~8x with its time ~2x, which LOWERS the aggregate
        # fraction although the step got faster.  For comparison with the records before it: the same time under the old credit.
        streamed = algorithmic_bytes("a3d_dmtet_count", {**dims, "dm_words_read": None})
        agg = roof["in_scope"]
        mb = agg["algorithmic_MB_per_step"] + (streamed / 1e6 - scope[cnt]["algorithmic_MB"]) * scope[cnt]["launches_per_step"]
        we, nwe, wt, nwt = dims["dm_words_read"]
        roof["dmtet_count_cull"] = dict(entry_point=cnt, edge_words_read=we, edge_words=nwe, tet_words_read=wt, tet_words=nwt,
                                        credited_MB=scope[cnt]["algorithmic_MB"], streamed_MB=round(streamed / 1e6, 3),
                                        in_scope_frac_if_credited_as_streamed=round(mb * 1e6 / (agg["us_per_step"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4))
    roof["fastest_in_scope"] = dict(kernel=top, achieved=scope[top]["GBps"], unit="GB/s", frac=round(scope[top]["GBps"] / HBM_PEAK_GBS, 4),
                                    launch_us=scope[top]["mean_us"])
    # model/networks side (out of scope): the field kernels, incl. the one compute-bound kernel of the library
    net = {k: v for k, v in kernels.items() if not k.startswith(IN_SCOPE + F3)}
    side = dict(us_per_step=round(sum(v["mean_us"] * v["launches_per_step"] for v in net.values()), 1))
    gemm = next((k for k in net if k.startswith("a3d_gemm_nn_relumask")), None)
    if gemm is not None:
        fl = algorithmic_flops(gemm, dims)
        tf = fl / (net[gemm]["mean_us"] * 1e-6) / 1e12
        side["mfma_gemm"] = dict(kernel=gemm, bound="mfma", achieved=round(tf, 1), peak=MFMA_FP32_PEAK_TFLOPS, unit="TFLOP/s",
                                 frac=round(tf / MFMA_FP32_PEAK_TFLOPS, 4), launch_us=net[gemm]["mean_us"], launches_per_step=net[gemm]["launches_per_step"])
    roof["networks_side"] = side
    return roof


def box_fingerprint(L, dev, scene_step=None, wall_ms_per_step=None):
    """What THIS box gives, so that a slow box and a regression can be told apart in a committed line: the shader / memory clocks the driver
    reports, a 92 MB streaming fill and read (the bytes the compositor writes per step; a3d_bw_probe_*, HIP events, best of 20), and --
    with ``scene_step`` -- the GPU-busy time of a step (sum of all kernel durations, torch.profiler over 3 steps) against its wall time:
    host_bound_frac = 1 - busy / wall is the share of the step during which the GPU waited for the host."""
    import subprocess

    fp = {"device": torch.cuda.get_device_name(dev)}
    fp["clocks_MHz"] = _clocks_mhz()
    ops_mod = importlib.import_module("3danimals_amd.ops")
    ops_mod.dispatch_order_ok(dev)  # (cached: the render path probed it on its first deferred resolve)
    fp["dispatch_order_probe"] = dict(ops_mod._dispatch_probe[torch.device(dev)],
                                      note="work-groups dispatched in linear-index order, the property the fused resolve's look-back rests on: "
                                           "16384 work-groups each waiting for the one 64 before it; status 2 = every wait ended")
    n = 92 * 1000 * 1000 // 16 * 4  # floats: 92 MB
    buf, sink = torch.empty(n, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.float32, device=dev)

    def best(fn):
        ts = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return min(ts)

    fill_ms = best(lambda: L.call("a3d_bw_probe_fill", L.ptr(buf), n, L.stream()))
    read_ms = best(lambda: L.call("a3d_bw_probe_read", L.ptr(buf), n, L.ptr(sink), L.stream()))
    fp["fill_92MB"] = dict(us=round(fill_ms * 1e3, 1), GBps=round(4 * n / fill_ms / 1e6, 1))
    fp["read_92MB"] = dict(us=round(read_ms * 1e3, 1), GBps=round(4 * n / read_ms / 1e6, 1))
    fp["note"] = ("fill / read: event time of ONE launch incl. its launch latency (~3 us); DESIGN.md section 4 measured 15.4 us = 6.3 TB/s for the fill "
                  "on the round-4 boxes")
    if scene_step is not None:
        try:
            from torch.profiler import ProfilerActivity, profile

            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3):
                    scene_step()
                torch.cuda.synchronize()
            busy_us = sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in prof.key_averages()) / 3.0
            fp["gpu_busy_ms_per_step"] = round(busy_us / 1e3, 3)
            if wall_ms_per_step:
                fp["wall_ms_per_step"] = round(wall_ms_per_step, 3)
                fp["host_bound_frac"] = round(max(0.0, 1.0 - busy_us / 1e3 / wall_ms_per_step), 4)
        except Exception as e:
            fp["gpu_busy_ms_per_step"] = f"unavailable ({type(e).__name__}: {str(e)[:80]})"
    return fp


def _clocks_mhz():
    """{sclk, mclk, fclk: MHz} as the driver reports them NOW: the starred row of pp_dpm_* in sysfs, else the "(NNNMhz)" of rocm-smi's
    clock lines -- frequencies, not DPM level indices (round 5 recorded the indices: VERDICT r5 weak 11)."""
    import glob
    import re
    import subprocess

    out = {}
    for name in ("sclk", "mclk", "fclk"):
        for path in sorted(glob.glob(f"/sys/class/drm/card*/device/pp_dpm_{name}")):
            try:
                rows = open(path).read().splitlines()
            except OSError:
                continue
            star = [r for r in rows if r.rstrip().endswith("*")]
            m = re.search(r"(\d+)\s*[Mm][Hh]z", star[0]) if star else None
            if m:
                out[name] = int(m.group(1))
                break
    if len(out) < 3:
        try:
            txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
            for name in ("sclk", "mclk", "fclk"):
                m = re.search(rf"{name} clock level:?\s*\d+:?\s*\((\d+)\s*[Mm][Hh]z\)", txt)
                if m and name not in out:
                    out[name] = int(m.group(1))
        except Exception as e:  # (best effort: the tool may be missing in a container)
            out.setdefault("note", f"rocm-smi unavailable ({type(e).__name__})")
    return out or "unavailable"


def parity_and_cpu_baseline(scene, args, threads):
    """One HIP step (weights untouched) -> (i) oracle/check.compare_step: STAGE-WISE parity at full size -- every stage re-done by the CPU
    oracle from the HIP output of the stage before it, per output, with the pixel of the maximum -- plus the end-to-end figure through
    the oracle's own chain; (ii) the CPU oracle's whole step on the first images of the SAME step, timed: the CPU baseline (1 warm-up +
    median of ``--cpu-runs``), whose per-term losses are compared too."""
    from oracle import check, step_ref

    torch.set_num_threads(threads)
    out = scene.step(backward=not args.forward_only, optimizer_step=False)
    torch.cuda.synchronize()
    n = max(1, min(args.cpu_sample_images, scene.frames))
    rep = check.compare_step(scene, out, n_images=n)
    st = step_ref.snapshot(scene, n)
    n = st["n"]
    runs = [step_ref.cpu_step(st, backward=not args.forward_only) for _ in range(1 + args.cpu_runs)]
    res = runs[-1]
    secs = sorted(r["seconds"] for r in runs[1:])
    sec = secs[len(secs) // 2]
    cpu = lambda t: t.detach().float().cpu()
    parity = dict(frames=n, resolution=list(scene.resolution), faces_equal=rep["faces_equal"], num_faces=rep["num_faces"])
    if rep["faces_equal"] and rep.get("geometry_only"):  # the step without rendering: the geometry stages are all there is
        parity.update(stages=dict(dmtet_vertices=rep["max_abs_vert_err"], prior_normals=rep["max_abs_prior_normal_err"], skinning=rep["max_abs_skin_err"],
                                  posed_normals=rep["max_abs_posed_normal_err"], posed_normal_err_vs_float64=rep["posed_normal_err_vs_float64"]),
                      loss_rel_err={k: round(abs(float(cpu(out["losses"][k])) - float(res["losses"][k])) / max(abs(float(res["losses"][k])), 1e-12), 7)
                                    for k in ("prior_normal_reg",)},  # (the other terms run over all frames here and over the CPU sample there)
                      note="no rendering in this step: DMTet index buffers bit-exact, vertices, skinning and both normals passes re-done by the CPU oracle "
                           "from the HIP output of the stage before")
        parity["pass"] = bool(rep["max_abs_vert_err"] == 0.0 and rep["max_abs_skin_err"] < 1e-5 and rep["max_abs_posed_normal_err"] < 1e-4)
        cpu_baseline = dict(value=round(n / sec, 4), unit="images/s", cores=threads, kind="port",
                            sample=f"oracle/step_ref.cpu_step fwd+bwd on {n} of the {scene.frames} frames (ponymation stage 2, no rendering: grid {grid_name(args)} DMTet, "
                                   f"deformation, LBS, normals), 1 warm-up + median of {args.cpu_runs} runs, torch {threads} threads of {os.cpu_count()} logical cores, "
                                   f"{sec:.1f} s per run")
        return parity, cpu_baseline
    if rep["faces_equal"]:
        stage_keys = [k for k in rep if k.endswith(("clip", "raster", "gbuffer", "gbuffer_flow"))]
        parity.update(
            raster_ids_equal=rep["raster_ids_equal"], max_abs_image_err=rep["max_abs_image_err"], images=rep["images"],
            stages=dict(dmtet_vertices=rep["max_abs_vert_err"], prior_normals=rep["max_abs_prior_normal_err"], skinning=rep["max_abs_skin_err"],
                        posed_normals=rep["max_abs_posed_normal_err"], **{k: rep[k] for k in stage_keys}),
            networks_cpu_vs_gpu=rep.get("fields"),
            end_to_end=dict(max_abs_image_err=rep["max_abs_image_err_end_to_end"], images=rep["end_to_end"],
                            frac_pixels_owner_flip=round(rep["frac_pixels_owner_flip"], 7)),
            note="stage-wise: each stage re-done by the CPU oracle from the HIP output of the previous stage (identical inputs, no pixel excluded; the "
                 "networks' GPU outputs injected, their own CPU-vs-GPU difference under networks_cpu_vs_gpu); end_to_end: the oracle's own chain "
                 "from the SDF values on (its own skinning, clip matmul and CPU networks), owner-flipped pixels excluded and counted")
        rel = {}
        for k, v in res["losses"].items():
            if k in out["losses"] and v.dim() >= 1 and v.shape[0] in (n, st["nb"]):
                a, b = float(cpu(out["losses"][k])[: v.shape[0]].mean()), float(v.mean())
                rel[k] = round(abs(a - b) / max(abs(b), 1e-12), 7)
        parity["loss_rel_err"] = rel
    parity["pass"] = check.passes(rep)
    cpu_baseline = dict(value=round(n / sec, 4), unit="images/s", cores=threads, kind="port",
                        sample=f"oracle/step_ref.cpu_step fwd+bwd on {n} of the {scene.frames} frames of this workload ({scene.workload}: grid {grid_name(args)} "
                               f"DMTet, LBS, {args.resolution}x{args.resolution} raster+shade+antialias, losses), 1 warm-up + median of {args.cpu_runs} runs, "
                               f"torch {threads} threads of {os.cpu_count()} logical cores, {sec:.1f} s per run")
    return parity, cpu_baseline


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run, one rank per GPU of this node
    (what `accelerate launch --multi_gpu run.py` does for the reference, /root/reference/README.md:49-52).  Everything the ranks write to
    stdout is passed on to stderr, except rank 0's JSON line, which is printed last -- the ONE line on stdout."""
    import socket
    import subprocess

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port",
           str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for raw in proc.stdout:
        text = raw.rstrip("\n")
        cand = None
        if text.startswith("{") and text.endswith("}"):
            try:
                cand = json.loads(text)
            except ValueError:
                cand = None
        if isinstance(cand, dict) and "metric" in cand:
            line = cand
        else:
            print(text, file=sys.stderr, flush=True)
    rc = proc.wait()
    if line is not None:
        line["launcher"] = "bench.py self-launch (torch.distributed.run, 127.0.0.1:%d)" % port
        print(json.dumps(line), flush=True)
    return rc if rc != 0 else (0 if line is not None else 1)


def dry_launch(args, rank, world):
    """The launch / rendezvous / collect plumbing without any GPU work (tests: 2 gloo ranks on CPU)."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    total = float(rank + 1)
    if world > 1:
        dist.init_process_group(args.backend)
        t = torch.tensor([total], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.barrier()
        dist.all_reduce(t)
        total, ranks = float(t.item()), dist.get_world_size()
        dist.barrier()
        dist.destroy_process_group()
    else:
        ranks = 1
    if rank == 0:
        print("rank 0: stdout chatter before the line goes to stderr under self-launch", flush=True)
        print(json.dumps({"metric": "train images/sec fwd+bwd @256x256 b16", "value": None, "unit": "images/s", "n_gpus": world, "dry_launch": True,
                          "rccl_ranks": ranks, "backend": args.backend, "allreduce_sum": total, "steps": args.steps, "warmup": args.warmup}), flush=True)
    return 0


def from_initial_state(scene, step_fn):
    """-> a step function whose every call starts from the state ``scene`` has now: its weights (copied back in place, so that captured
    HIP graphs keep their pointers) and its optimiser state as the first call creates it (Adam creates every entry -- step, moments --
    as zeros).  The backward's float atomics round differently from run to run; carried from step to step, Adam and the DMTet level
    set amplify that into other meshes, covered pixels and images (profiles/r07_dump_reproducibility.json).  Started from the same
    state, consecutive steps still differ -- the grid jitter (and Fauna's random-view azimuths) are drawn from the global generator on
    every call -- but the n-th step of one run and the n-th step of another do the same work on the same inputs.  The restore runs
    inside the timed interval: 21-23 us per step on an MI355X (one foreach copy of 6.8 MB of weights, one foreach zero of the Adam state),
    0.15 % of a 15.5 ms step (profiles/r07_dump_reproducibility.json)."""
    params = [p for p in scene.parameters()]
    initial = [p.detach().clone() for p in params]
    state = []

    def run():
        if state:
            with torch.no_grad():
                torch._foreach_copy_(params, initial)
                for group in state:
                    torch._foreach_zero_(group)
        out = step_fn()
        if not state:  # the first call created the optimiser state: zeroed before every later call
            by_device = {}
            for s in scene.optimizer.state.values():
                for t in s.values():
                    if torch.is_tensor(t):
                        by_device.setdefault(t.device, []).append(t)
            state.extend(by_device.values())
        return out

    return run


DUMP_SAMPLE = 1 << 21  # elements kept of a larger output (8 MB in float32); a step hands back at most four such arrays
DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out, dirname):
    """--dump-outputs: every tensor of a step's output dict (nested dicts flattened as <key>_<name>) -> DIR/<name>.npy.  Returns
    {name: {shape, sampled}} for the result line."""
    import numpy as np

    flat = {}
    for k, v in out.items():
        for kk, vv in (v.items() if isinstance(v, dict) else [(None, v)]):
            if torch.is_tensor(vv):
                flat[k if kk is None else f"{k}_{kk}"] = vv.detach()
    os.makedirs(dirname, exist_ok=True)
    written, total = {}, 0
    for name, t in sorted(flat.items()):
        values = t.reshape(-1)
        sampled = values.numel() > DUMP_SAMPLE
        if sampled:  # fixed, seeded indices: the same elements in every run of the same shape
            idx = torch.randint(values.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            values = values[idx.to(values.device)]
        arr = values.cpu().numpy().astype(np.float64 if t.dtype == torch.float64 else np.float32, copy=False)
        if not sampled:
            arr = arr.reshape(tuple(t.shape))
        total += arr.nbytes
        if total > DUMP_BUDGET_BYTES:
            raise RuntimeError(f"--dump-outputs: more than {DUMP_BUDGET_BYTES >> 20} MB at '{name}'")
        np.save(os.path.join(dirname, name + ".npy"), arr)
        written[name] = dict(shape=list(t.shape), sampled=DUMP_SAMPLE if sampled else None)
    return written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure everything beside the headline: extra legs, "
                    "rank diagnostics, per-kernel roofline, launch attribution, box fingerprint, host synchronisations, CPU-oracle parity and "
                    "baseline, drop-in networks, BASELINE configs[1] (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--carry-state", action="store_true", help="time the training trajectory: weights and Adam state carried from step to "
                    "step (the mesh drifts as the synthetic training goes on; what the committed lines and profiles measure).  Two runs "
                    "of the same arguments then diverge beyond rounding (the backward's float atomics, amplified from step to step).  "
                    "Default: every warm-up and timed step starts from the initial state (from_initial_state)")
    ap.add_argument("--batch", type=int, default=None, help="images (sequences for ponymation) per GPU; default 16 (8 sequences)")
    ap.add_argument("--frames", type=int, default=8, help="frames per sequence (ponymation only)")
    ap.add_argument("--grid-res", type=int, default=64)
    ap.add_argument("--grid", default=None, help="a named tet grid instead of the Kuhn grid of --grid-res cells: bcc51s / bcc102s = BCC lattices "
                    "(Quartet's family) of the reference's '128' / '256' class in a random numbering (tetgrid.named_grid)")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--workload", choices=("magicpony", "fauna", "ponymation"), default="magicpony")
    ap.add_argument("--networks", choices=("fast", "reference", "both"), default="both",
                    help="fast: the output-identical field evaluation of hostnets (headline); reference: model/networks' own formulation "
                         "(per-point feature concat, per-call frequency upload, no TunableOp, no fused kernels); both: headline = fast, and "
                         "with --full the reference formulation is measured too (single GPU only) and reported under 'dropin'")
    ap.add_argument("--seed", type=int, default=0, help="seed of the synthetic scene's networks, cameras and poses (0: every committed line but the "
                    "long Fauna run, whose random trajectory empties a leg quadrant at seed 0: estimate_bones then raises where the "
                    "reference drops into pdb, skinning.py:183)")
    ap.add_argument("--mesh", choices=("quadruped", "spiky"), default="quadruped", help="spiky: the trained-like mesh (pipeline.synthetic_spikes: the "
                    "quadruped with a percent of its vertices pulled into thin spikes, tuned to the step-600 statistics of the long run); the default "
                    "line carries it as extra_legs.spiky anyway")
    ap.add_argument("--no-spiky-leg", action="store_true", help="skip the extra leg on the trained-like mesh (default line, 1 GPU, magicpony)")
    ap.add_argument("--no-fingerprint", action="store_true", help="skip the box fingerprint (clocks, 92 MB fill / read probe, GPU-busy time per step)")
    ap.add_argument("--no-render", action="store_true", help="ponymation only: the step config/train_ponymation_horse_stage2.yaml really runs (enable_render "
                    "false; combine with --batch 20 --frames 10): DMTet + instance deformation + [B,F] LBS + the make_mesh passes on B x F meshes + backward, "
                    "no rasteriser")
    ap.add_argument("--no-attribution", action="store_true", help="skip the launch attribution (tools/glue_attribution.py: every GPU kernel of 3 steps "
                    "attributed to the code that launched it -- the path's entry points, the torch kernels its own modules launch, networks, ...)")
    ap.add_argument("--no-deform", action="store_true", help="magicpony without the instance deformation (the round-1 step)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU oracle (parity and cpu_baseline = null)")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the HIP-event per-kernel pass (roofline = null); for PMC runs")
    ap.add_argument("--no-tuned-gemms", action="store_true", help="do not load the shipped TunableOp results for the torch MLPs")
    ap.add_argument("--forward-only", action="store_true", help="BASELINE configs[1] (test_magicpony_horse): forward passes under no_grad, no "
                    "backward, no optimiser; combine with --batch 8")
    ap.add_argument("--cpu-sample-images", type=int, default=4)
    ap.add_argument("--cpu-runs", type=int, default=3)
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="torch.distributed backend for --gpus > 1 (nccl = RCCL over xGMI; gloo "
                    "only for the launch-plumbing tests)")
    ap.add_argument("--share-gpu", action="store_true", help="every rank on cuda:0 (gloo only: exercises the N-rank path on a 1-GPU box)")
    ap.add_argument("--dry-launch", action="store_true", help="launch plumbing only: rendezvous, barrier, one all-reduce, the JSON line; no GPU work")
    ap.add_argument("--per-rank-poses", action="store_true", help="different poses / cameras per rank (unequal covered-pixel counts) instead of "
                    "the equal-work default")
    ap.add_argument("--no-rank-diagnostics", action="store_true", help="--gpus N > 1 only: skip the per-rank host-side figures (blocking read-backs per step, "
                    "GPU-busy time of the rank's own kernels against its wall time per step)")
    ap.add_argument("--no-extra-legs", action="store_true", help="--gpus N > 1 only: skip the two extra timed legs of the line (per-rank poses; the "
                    "Fauna per-rank step) that follow the headline leg")
    args = ap.parse_args()
    assert not args.no_render or args.workload == "ponymation", "--no-render is the ponymation stage-2 configuration"
    assert args.steps >= 1 and args.warmup >= 0, "--steps >= 1, --warmup >= 0"
    full = args.full

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:  # plain `python bench.py --gpus N`: spawn the ranks ourselves
        sys.exit(self_launch(args.gpus))

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}"
    if args.dry_launch:
        return dry_launch(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs an MI355X; the HIP hot path has no CPU fallback"
    assert not args.share_gpu or args.backend == "gloo", "two RCCL ranks cannot share a device: --share-gpu needs --backend gloo"
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    L = importlib.import_module("3danimals_amd._lib")
    L.lib()  # fail loudly, now, if the HIP library is missing
    headline_networks = "reference" if args.networks == "reference" else "fast"
    tuned = False
    if headline_networks == "fast" and not args.no_tuned_gemms:
        tuned = importlib.import_module("3danimals_amd.gemm_tuning").enable()
    hostnets.reference_formulation(headline_networks == "reference")

    batch = args.batch if args.batch is not None else (8 if args.workload == "ponymation" else 16)
    frames = args.frames if args.workload == "ponymation" else 1

    def make_scene(workload=args.workload, per_rank_poses=args.per_rank_poses, mesh=args.mesh):
        b = batch if (workload == args.workload or args.workload != "ponymation") else 16  # (ponymation's --batch counts sequences)
        return pipeline.SyntheticScene(grid=args.grid, grid_res=args.grid_res, batch=b, resolution=(args.resolution, args.resolution), device=dev, seed=args.seed,
                                       data_seed=1000 * rank + args.seed, workload=workload, num_frames=frames if workload == "ponymation" else 1,
                                       deform=((workload == "magicpony" or (workload == "ponymation" and args.no_render)) and not args.no_deform),
                                       pose_seed=(rank if per_rank_poses else 0), mesh=mesh, render=not (args.no_render and workload == "ponymation"))

    scene = make_scene()
    scene.netShape.capture_sdf_gradient_graph()  # HIP graphs are captured before any RCCL thread exists; the steps only replay them
    # --gpus N > 1: two more timed legs ride in the same line (and the same launch), so that the first multi-GPU record also says what
    # the equal-work headline cannot: (i) every rank on its OWN poses / cameras (unequal covered-pixel counts: the slowest rank sets the
    # step), (ii) the Fauna per-rank step (bones re-estimated in the step, two renders: 4 host read-backs per step on every rank --
    # where eight Python processes stalling at different moments would show; Trainer.py:170-179,304-308, Fauna.py:111-173).  Their
    # scenes (and HIP graphs) exist before the process group does, like the headline's.
    extra_scenes = {}
    if full and world > 1 and not args.no_extra_legs and not args.forward_only:
        if not args.per_rank_poses:
            extra_scenes["per_rank_poses"] = make_scene(per_rank_poses=True)
        if args.workload != "fauna":
            extra_scenes["fauna"] = make_scene(workload="fauna")
        for sc in extra_scenes.values():
            sc.netShape.capture_sdf_gradient_graph()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group("gloo")
    # weak scaling = fixed work per GPU: every rank renders the same poses / cameras (hence the same number of covered pixels and
    # the same GEMM shapes) against its own image features and target images, so the all-reduced gradients differ per rank.
    module = None
    if world > 1:
        module = torch.nn.parallel.DistributedDataParallel(scene, device_ids=[local_rank], broadcast_buffers=False, gradient_as_bucket_view=True)
    train = not args.forward_only
    if not train:
        module = None  # forward only: nothing to all-reduce; the ranks are independent replicas

    # W untimed warm-up steps, then exactly K steps bracketed by barrier + synchronize on both sides, MAX over ranks
    du = importlib.import_module("3danimals_amd.dist_util")
    tdev = dev if (world == 1 or args.backend == "nccl") else "cpu"
    calls, last_out = [0], {}
    train_step = lambda: scene.step(module=module, backward=train)
    same_step = train_step if args.carry_state else from_initial_state(scene, train_step)

    def headline_step():
        out = same_step()
        calls[0] += 1
        if args.dump_outputs and calls[0] == args.warmup + args.steps:  # the last timed step: what its caller receives
            last_out.update(out)

    elapsed, rank_seconds = du.timed_steps(headline_step, args.steps, args.warmup, device=dev, per_rank=True)
    images = world * scene.frames * args.steps
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dict(dir=args.dump_outputs, arrays=dump_outputs(last_out, args.dump_outputs))
    last_out.clear()

    def covered_of(sc):
        c = int((sc.last["rast"][..., 3] > 0).sum()) if "rast" in sc.last else 0
        if world == 1:
            return [c]
        t = torch.zeros(world, dtype=torch.int64, device=tdev)
        t[rank] = c
        dist.all_reduce(t)
        return [int(v) for v in t.tolist()]

    extra_legs = {}
    for name, sc in extra_scenes.items():  # (every rank runs the same legs in the same order)
        mod = torch.nn.parallel.DistributedDataParallel(sc, device_ids=[local_rank], broadcast_buffers=False, gradient_as_bucket_view=True)
        t, per_rank = du.timed_steps(lambda: sc.step(module=mod, backward=True), args.steps, args.warmup, device=dev, per_rank=True)
        extra_legs[name] = dict(value=round(world * sc.frames * args.steps / t, 3), unit="images/s", ms_per_step=round(t / args.steps * 1e3, 3),
                                ms_per_step_per_rank=[round(v / args.steps * 1e3, 3) for v in per_rank], covered_pixels_per_rank=covered_of(sc),
                                workload=sc.workload, batch_per_gpu=sc.batch, steps=args.steps, warmup=args.warmup)
        del mod
    extra_scenes.clear()

    # ---- per-rank host-side figures of the N-rank run (round 6): SURVEY 8e names the host as the scaling risk -- N Python processes each
    # issuing ~600 launches per step and stalling at their own read-backs.  Every rank: blocking synchronisations in one step (torch's
    # sync-debug hook) and the GPU time of ITS OWN kernels over two steps against their wall time; gathered, so that the line shows them.
    rank_diag = None
    if full and world > 1 and not args.no_rank_diagnostics:
        import warnings

        from torch.profiler import ProfilerActivity, profile

        step_fn = lambda: scene.step(module=module, backward=train)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                step_fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        n_sync = sum(1 for w in caught if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message))
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(2):
                step_fn()
            torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) / 2 * 1e3
        busy_ms = sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in prof.key_averages()) / 2e3
        mine = dict(rank=rank, host_syncs_per_step=n_sync, own_kernels_ms_per_step=round(busy_ms, 3), wall_ms_per_step_under_profiler=round(wall_ms, 3),
                    host_bound_frac=round(max(0.0, 1.0 - busy_ms / wall_ms), 4), cpu_affinity=len(os.sched_getaffinity(0)))
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        rank_diag = dict(per_rank=gathered, note="host_bound_frac = 1 - (GPU time of the rank's own kernels) / (its wall time per step, profiler on); with "
                         "--share-gpu every rank's kernels queue behind the others' on ONE device, so 1 - N x own / wall is what the device idles")

    def dims_of(sc):
        prior = sc.last["prior"]
        return dict(B=sc.frames, V=int(prior.v_pos.shape[1]), F=int(prior.t_pos_idx.shape[1]), H=args.resolution, W=args.resolution,
                    Nv=int(sc.netShape.verts.shape[0]), Ne=int(sc.netShape.topology.edges32.shape[0]),
                    Nt=int(sc.netShape.topology.tets32.shape[0]), K=int(sc.bones.shape[2]),
                    P=int((sc.last["rast"][..., 3] > 0).sum()) if "rast" in sc.last else 0,
                    dm_words_read=sc.netShape.topology.words_read(sc.netShape.current_sdf),
                    skin_v_batch=sc.frames if getattr(sc, "deform", False) else 1,  # (instance deformation: rest vertices per image)
                    cover_blocks=_cover_blocks(sc.last["rast"]) if "rast" in sc.last else 0)

    # ---- per-kernel timing pass (same workload, separate from the headline timing so the events do not perturb it)
    roofline, kernels = None, {}
    if full and rank == 0 and not args.no_kernel_timing:
        kernels, dims = kernel_pass(scene, module, L, min(args.steps, 10), world, dims_of, train)
        roofline = roofline_of(kernels, dims, workload_signature(args, batch))

    # ---- the trained-like mesh as an extra leg of the default line: the 25-step-old near-ellipsoid is the cheapest mesh
    # this path will ever see; the reference trains for 1e5 iterations (config/model/magicpony.yaml:31-33).  Same step, same networks, the
    # spiky mesh: images/s, in-scope time, and the two calls whose cost follows depth complexity and silhouette length.
    if (full and rank == 0 and world == 1 and train and args.workload == "magicpony" and args.mesh == "quadruped" and not args.no_spiky_leg
            and not args.no_kernel_timing):
        sp = make_scene(mesh="spiky")
        sp_steps = max(5, min(args.steps, 20))
        ev0 = dict(importlib.import_module("3danimals_amd.ops").resolve_events)
        t = du.timed_steps(lambda: sp.step(backward=True), sp_steps, 3, device=dev)
        sp_kernels, sp_dims = kernel_pass(sp, None, L, min(sp_steps, 10), 1, dims_of, True)
        agg = _aggregate(sp_kernels, IN_SCOPE)
        pick = lambda pre: next((round(v["mean_us"], 2) for k, v in sp_kernels.items() if k.startswith(pre)), None)
        box = _pixel_boxes(sp)
        extra_legs["spiky"] = dict(value=round(sp.frames * sp_steps / t, 3), unit="images/s", ms_per_step=round(t / sp_steps * 1e3, 3), steps=sp_steps,
                                   in_scope_us_per_step=agg["us_per_step"], in_scope_frac=agg["frac"], rast_fwd_us=pick("a3d_rast_fwd"),
                                   composite_aa_fwd_us=pick("a3d_composite_aa_fwd"), composite_aa_bwd_us=pick("a3d_composite_aa_bwd"),
                                   gbuffer_bwd_us=pick("a3d_gbuffer_bwd"), mesh=dict(V=sp_dims["V"], F=sp_dims["F"], P=sp_dims["P"], **box),
                                   headline_mesh=_pixel_boxes(scene),
                                   resolve_events={k: v - ev0.get(k, 0) for k, v in importlib.import_module("3danimals_amd.ops").resolve_events.items()},
                                   note="pipeline.SPIKES; the long run it stands for, step 600 (profiles/r04_long_run_diag.txt): box mean 35.7, max 9375, "
                                        "3.07e5 covered pixels")
        del sp

    # ---- who launched what (round 6): in_scope_us_per_step above sums the C-ABI entry points only; the torch kernels the path's own
    # modules launch (copies, slices and their padded gradients, accumulations) belong to the path too.  torch.profiler, 3 steps.
    attribution = None
    if full and rank == 0 and world == 1 and not args.no_attribution and not args.no_kernel_timing:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import glue_attribution

            attribution = glue_attribution.profile_steps(lambda: scene.step(backward=train), 3)
        except Exception as e:  # (a profiler that cannot start must not cost the line)
            attribution = dict(error=f"{type(e).__name__}: {str(e)[:200]}")

    fingerprint = None
    if full and rank == 0 and not args.no_fingerprint:
        fingerprint = box_fingerprint(L, dev, (lambda: scene.step(module=module, backward=train)) if world == 1 else None, elapsed / args.steps * 1e3)

    # ---- blocking host <-> device synchronisations inside one steady-state step (torch's sync-debug hook; sizes that shapes depend on)
    host_syncs = None
    if full and rank == 0 and world == 1:
        import warnings

        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                scene.step(backward=train)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        sites = [str(w.message).split("(Triggered")[0].strip()[:80] + f" @ {os.path.basename(w.filename)}:{w.lineno}" for w in caught
                 if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message)]
        host_syncs = dict(per_step=len(sites), sites=sorted(set(sites)))

    threads = min(os.cpu_count(), 32)  # torch-CPU stops scaling (and thrashes) far below the 256 logical cores of the GPU box
    parity = cpu_baseline = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        parity, cpu_baseline = parity_and_cpu_baseline(scene, args, threads)

    # ---- the drop-in figure: the same step with model/networks evaluated the reference's own way (what a maintainer gets who
    # overlays only model/geometry + model/render).  Single GPU only; a fresh scene, since Adam state is per formulation.
    dropin = None
    if full and rank == 0 and world == 1 and args.networks == "both":
        hostnets.reference_formulation(True)
        tunable_was = torch.cuda.tunable.is_enabled()
        torch.cuda.tunable.enable(False)
        ref_scene = make_scene()
        ref_steps = max(3, min(args.steps, 10))
        t = du.timed_steps(lambda: ref_scene.step(backward=train), ref_steps, 2, device=dev)
        dropin = dict(networks="reference formulation: per-point feature concatenation (MLPs.py:84-90), frequency table uploaded in every forward "
                               "(HarmonicEmbedding.py:41), one plain Linear per layer, no TunableOp table, no HIP field kernels; hot path unchanged",
                      value=round(ref_scene.frames * ref_steps / t, 3), unit="images/s", ms_per_step=round(t / ref_steps * 1e3, 3), steps=ref_steps)
        hostnets.reference_formulation(False)
        torch.cuda.tunable.enable(tunable_was)
        del ref_scene

    config1 = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.workload == "magicpony":
        # BASELINE config 1 (geometry only, no raster): CPU oracle beside the HIP path on the same inputs
        from oracle import geometry_ref

        dmtet_mod = importlib.import_module("3danimals_amd.model.geometry.dmtet")
        inp = geometry_ref.make_inputs(res=32, batch=16, seed=0)
        for _ in range(2):
            geometry_ref.cpu_step(inp)
        cpu_s = sorted(geometry_ref.cpu_step(inp)["seconds"] for _ in range(5))[2]
        gin = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
        topo = dmtet_mod.TetGridTopology(gin["tets"])
        for _ in range(3):
            res1 = pipeline.geometry_config1_step(gin, topo)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(20):
            pipeline.geometry_config1_step(gin, topo)
        torch.cuda.synchronize()
        hip_s = (time.perf_counter() - t1) / 20
        config1 = dict(workload="DMTet (Kuhn R=32) + normals + estimate_bones + LBS (B=16, K=20) + normals, fwd+bwd, no raster",
                       mesh=dict(V=res1["V"], F=res1["F"]), cpu_port_ms=round(cpu_s * 1e3, 2), cpu_images_per_s=round(16 / cpu_s, 1),
                       cpu_threads=threads, hip_ms=round(hip_s * 1e3, 3), hip_images_per_s=round(16 / hip_s, 1),
                       note="estimate_bones (host logic with read-backs, once per epoch in training) is inside both timings")

    # what every rank rendered (covered pixels decide the MLP work): gathered so the line shows the balance across ranks
    covered_per_rank, ranks = covered_of(scene), (dist.get_world_size() if world > 1 else 1)

    if rank == 0:
        what = {"magicpony": "train_magicpony_horse-like synthetic step: DMTet(%s)+deformation+LBS(20 bones)+3x make_mesh+raster/interp/antialias "
                             "+ SDF/texture/DINO/light/deform MLPs + photometric/mask/DINO losses + regularisers, fwd+bwd+Adam" % grid_name(args),
                "fauna": "train_fauna per-rank synthetic step: conditioned SDF (CoordMLP_Mod, 128-d embedding) + DMTet(%s) + bones re-estimated "
                         "every iteration (bone_y_threshold 0.4) + LBS + main render + random-view mask render + losses, fwd+bwd+Adam" % grid_name(args),
                "ponymation": ("train_ponymation stage 2 as configured (enable_render false, train_ponymation_horse_stage2.yaml:16-27): DMTet(%s) + instance "
                               "deformation + [B,F] LBS + make_mesh (vertex normals) of B*F meshes, teacher / regulariser losses + a linear functional of the "
                               "posed meshes (so that the path's backward runs), fwd+bwd+Adam" % grid_name(args)) if args.no_render else
                              ("train_ponymation stage-2-like synthetic step with rendering: DMTet(%s) + [B,F] LBS + B*F frames rendered with "
                               "'shaded','dino_pred','flow' + photometric/mask/DINO/flow losses, fwd+bwd+Adam" % grid_name(args))}[args.workload]
        line = {
            "metric": "train images/sec fwd+bwd @256x256 b16" if train else "test images/sec forward only @256x256 b8 (BASELINE configs[1])",
            "value": round(images / elapsed, 3),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "rccl_ranks": ranks,
            "backend": ("rccl" if args.backend == "nccl" else args.backend) if world > 1 else None,
            "covered_pixels_per_rank": covered_per_rank,
            "ms_per_step_per_rank": [round(v / args.steps * 1e3, 3) for v in rank_seconds],
            "extra_legs": extra_legs or None,
            "rank_diagnostics": rank_diag,
            "scaling_curve_note": None if world == 1 else ("no N > 1 RCCL scaling curve has been measured on hardware yet (no multi-GPU node was "
                                                            "available to the driver in rounds 1-5); this line is ONE point, efficiency is the driver's to compute"),
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "full": full,  # False: the objects below that --full measures are null
            "carry_state": bool(args.carry_state),  # True: a training trajectory; False: every step from the initial state
            "dump_outputs": dumped,
            "config": {"workload": what, "name": args.workload, "batch_per_gpu": batch, "frames_per_sequence": frames, "global_batch": world * batch,
                       "resolution": [args.resolution, args.resolution], "grid": grid_name(args), "mesh": args.mesh, "seed": args.seed, "dmtet_pass": getattr(scene.netShape.topology, "_last_count_pass", None), "parallelism": f"dp{world}",
                       "networks": headline_networks, "tuned_mlp_gemms": bool(tuned),
                       "mode": "train (fwd+bwd+Adam)" if train else "forward only (no_grad)", "render": not args.no_render,
                       "per_rank_data": ("per-rank poses/cameras, image features and targets (covered pixels differ per rank)" if args.per_rank_poses else
                                         "same poses/cameras on every rank (equal work per GPU: covered-pixel imbalance across ranks is NOT in this "
                                         "figure), per-rank image features and targets")},
            # (scalars lifted to the top level so that a record that keeps only top-level scalars still has them)
            "dmtet_pass": getattr(scene.netShape.topology, "_last_count_pass", None),
            "in_scope_us_per_step": None if not roofline or not roofline.get("in_scope") else roofline["in_scope"]["us_per_step"],
            "in_scope_frac": None if not roofline or not roofline.get("in_scope") else roofline["in_scope"]["frac"],
            "in_scope_frac_bytes_weighted": None if not roofline or not roofline.get("in_scope") else roofline["in_scope"]["frac_bytes_weighted"],
            "in_scope_calls_per_step": None if not roofline or not roofline.get("in_scope") else roofline["in_scope"]["entry_point_calls_per_step"],
            # (round 6) the path's GPU time as the profiler attributes it: kernels of the in-scope entry points + the torch kernels launched
            # from inside the path's own modules (model/geometry, model/render, ops.py) -- THE figure to compare across rounds from now on
            # (first honest value, same step before the glue was removed: 212 + 380 = 591 us, profiles/r06_glue_before.json)
            "in_scope_glue_us_per_step": None if not attribution or "error" in attribution else attribution["in_scope_glue_us_per_step"],
            "in_scope_total_us_per_step": None if not attribution or "error" in attribution else attribution["in_scope_total_us_per_step"],
            "dropin_images_per_s": None if dropin is None else dropin["value"],
            "parity_pass": None if parity is None else bool(parity.get("pass")),
            "box": fingerprint,
            # fused resolve + covered-pixel list + G-buffer launches of this process: how many took the one-launch path, how many outgrew the
            # rows sized from the previous frame (+25 %) and re-ran the exact two-launch half, stand-alone resolves, look-back timeouts
            "resolve_events": dict(importlib.import_module("3danimals_amd.ops").resolve_events),
            "roofline": roofline,
            "attribution": attribution,
            "host_syncs": host_syncs,
            "parity": parity,
            "dropin": dropin,
            "cpu_baseline": cpu_baseline,
            "config1_geometry": config1,
            "kernels": kernels,
        }
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:  # the ONE json line is the last thing written to stdout (after RCCL's own start-up / tear-down chatter)
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
