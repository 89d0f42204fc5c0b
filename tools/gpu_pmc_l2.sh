#!/bin/bash
# FETCH_SIZE, WRITE_SIZE and L2 hit / miss passes of the default bench (separate rocprofv3 runs, --kernel-trace only, per the guide:
# FETCH_SIZE and WRITE_SIZE do not fit the L2's four counters together) for the library in BFCNN_HIP_LIB, or the package's own:
#   BFCNN_HIP_LIB=$PWD/blind_image_denoising_amd/lib/variants/libbfcnn_hip_L2S16.so bash tools/gpu_pmc_l2.sh L2S16
#   ->  $PMC_OUT/pmc_l2_<name>/summary.txt   (PMC_OUT: where the logs and the summary go; default build/, which git ignores)
set -uo pipefail
name="${1:-default}"
repo="$PWD"
out="${PMC_OUT:-$repo/build}/pmc_l2_$name"; mkdir -p "$out"
out="$(cd "$out" && pwd)"                            # the passes run from /tmp: a relative PMC_OUT must still point here
export TMPDIR=/tmp
raw="$(mktemp -d /tmp/pmc_l2_XXXXXX)"
for c in FETCH_SIZE WRITE_SIZE "TCC_HIT_sum TCC_MISS_sum"; do
    tag="${c%% *}"
    ( cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --pmc $c --output-format csv -d "$raw/$tag" -- \
        python "$repo/bench.py" --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline ${BENCH_ARGS:-} > "$out/$tag.log" 2>&1 ) ||
        { echo "pass $tag failed"; tail -n 5 "$out/$tag.log"; exit 1; }
done
python tools/pmc_summary.py "$raw" | tee "$out/summary.txt"
