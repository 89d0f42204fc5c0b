#!/bin/bash
# A/B builds of the activation stream's cache policy (csrc/h3v_core.h): every H3_LOAD_POLICY x H3_STORE_POLICY combination of the pair
# kernel, with the head's loads plain ("LxSy") and nt ("LxSyH2"), linked with the current objects of the other units (run csrc/build.sh
# first).   tools/stream_policy_variants.sh   ->  lib/variants/libbfcnn_hip_L<l>S<s>[H2].so
# (one unit and one macro: tools/ablate_unit.sh; this script exists because a combination sets two macros in two units)
set -euo pipefail
cd "$(dirname "$0")/.."
src=blind_image_denoising_amd/csrc
obj=blind_image_denoising_amd/lib/obj
out=blind_image_denoising_amd/lib/variants
mkdir -p "$out"
[ -f "$obj/.units" ] || { echo "run blind_image_denoising_amd/csrc/build.sh first ($obj/.units is missing)" >&2; exit 1; }
cc=(/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-pass-failed)
pids=()
for l in 0 2; do for s in 0 2 16 18; do
    "${cc[@]}" -DH3_LOAD_POLICY=$l -DH3_STORE_POLICY=$s -c $src/fused_h3w.hip -o "$out/fused_h3w_L${l}S${s}.o" & pids+=($!)
done; done
for h in 0 2; do
    "${cc[@]}" -DH3_LOAD_POLICY=$h -c $src/edge_layers.hip -o "$out/edge_layers_H${h}.o" & pids+=($!)
done
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ "$fail" -eq 0 ] || { echo "a variant failed to build" >&2; exit 1; }
others=()
while IFS= read -r u; do [ "$u" = fused_h3w ] || [ "$u" = edge_layers ] || others+=("$obj/$u.o"); done < "$obj/.units"
for l in 0 2; do for s in 0 2 16 18; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "${others[@]}" "$out/fused_h3w_L${l}S${s}.o" "$out/edge_layers_H0.o" -ldl \
        -o "$out/libbfcnn_hip_L${l}S${s}.so"
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "${others[@]}" "$out/fused_h3w_L${l}S${s}.o" "$out/edge_layers_H2.o" -ldl \
        -o "$out/libbfcnn_hip_L${l}S${s}H2.so"
done; done
ls -la "$out"/libbfcnn_hip_L*.so
