#!/bin/bash
# every committed bench line of a round (run on the GPU box from the repo root):  bash tools/run_bench_lines.sh <tag>
TAG=${1:-r06}
mkdir -p gpurun_out
run() { name=$1; shift; python bench.py "$@" > gpurun_out/${TAG}_bench_${name}.json 2> gpurun_out/${TAG}_bench_${name}.err || (echo "$name FAILED"; tail -5 gpurun_out/${TAG}_bench_${name}.err); tail -c 300 gpurun_out/${TAG}_bench_${name}.json | head -c 0; echo "$name done"; }
run default --full --carry-state
run fwd_b8_grid64 --full --carry-state --forward-only --batch 8 --networks fast
run fwd_b8_grid128 --full --carry-state --forward-only --batch 8 --networks fast --grid-res 128 --cpu-sample-images 2 --cpu-runs 1
run grid128 --full --carry-state --grid-res 128 --networks fast --cpu-sample-images 2 --cpu-runs 1
run fauna --full --carry-state --workload fauna --networks fast
run ponymation --full --carry-state --workload ponymation --networks fast --cpu-sample-images 8 --cpu-runs 1
# (round 4) the reference's real grid class in a file's arbitrary numbering: the "128" class in the training step and forward only, the "256" class forward only
run bcc51s --full --carry-state --grid bcc51s --networks fast
run fwd_b8_bcc51s --full --carry-state --grid bcc51s --forward-only --batch 8 --networks fast
run fwd_b8_bcc102s --full --carry-state --grid bcc102s --forward-only --batch 8 --networks fast --cpu-sample-images 2 --cpu-runs 1
# the long run: 400 timed steps after 100 of warm-up (the mesh the synthetic training drifts into; README quotes it beside the 25-step figure)
run long400 --full --carry-state --steps 400 --warmup 100 --networks fast --no-cpu-baseline
# The Fauna step on random targets is a chaotic trajectory that passes within ONE vertex of an empty leg quadrant (profiles/r05_fauna_quadrants.txt:
# 1 vertex around step 50); float atomics decide on which side a run falls, and when a quadrant empties estimate_bones raises, as the
# reference stops in pdb (skinning.py:183).  Such a run says nothing about 500 steps of the path: it is repeated, the attempts are counted.
for attempt in 1 2 3; do
  run long400_fauna --full --carry-state --workload fauna --steps 400 --warmup 100 --networks fast --no-cpu-baseline
  [ -s gpurun_out/${TAG}_bench_long400_fauna.json ] && break
  echo "long400_fauna: attempt $attempt emptied a leg quadrant" >> gpurun_out/${TAG}_long400_fauna_attempts.txt
done
# (round 5) ponymation stage 2 as configured: 20 sequences x 10 frames, enable_render false (train_ponymation_horse_stage2.yaml:16-27); the trained-like mesh as the headline
run ponymation_norender --full --carry-state --workload ponymation --no-render --batch 20 --frames 10 --networks fast --cpu-sample-images 20 --cpu-runs 1
run spiky --full --carry-state --mesh spiky --networks fast
# (round 6) eight ranks on ONE GPU (gloo): the N = 8 launch path and the host-side contention of eight Python processes, measured; no scaling claim
run ranks8_one_gpu --full --carry-state --gpus 8 --backend gloo --share-gpu --steps 10 --warmup 3 --no-cpu-baseline --no-fingerprint
