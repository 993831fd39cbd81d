#!/bin/bash
# Build libxhist_amd.so in-tree for gfx950 (cross-compiles without a GPU).  Twenty-three translation units (xhist_hot: the small code object a first call loads),
# compiled in parallel: nine that instantiate the float64 / float32 / mixed-dtype vector, routing and exchange kernels, the per-bin extrema and the positions of histogram_argextrema (xhist_extrema), the per-bin mean and variance with the third and fourth moments of histogram_skew_kurt (xhist_meanvar) and their weighted form (xhist_meanvar_w), the per-bin quantiles (xhist_quantile) and their weighted form (xhist_quantile_w), the per-bin covariance of two value arrays (xhist_cov) and its weighted form (xhist_cov_w), the per-sample maps bin_index, histogram_lookup and histogram_anomaly (xhist_map), the order-independent per-bin sums (xhist_sum), the stable group-by of the samples by bin (xhist_group), the samples grouped by bin and sorted by value inside each bin (xhist_sort), the rank of every sample's value inside its bin and, in the same unit because it shares that unit's kernels, the per-bin mode of histogram_mode, the per-bin distinct values of bin_unique and their weighted twins (xhist_rank, which includes xhist_rank.hip.h, xhist_mode.hip.h, xhist_unique.hip.h and xhist_wruns.hip.h), and the rest.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${XHIST_BUILD_OUT:-$here/../libxhist_amd.so}"  # (development: XHIST_BUILD_OUT / XHIST_BUILD_FLAGS build an A/B variant next to the library)
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
obj="$(mktemp -d)"
trap 'rm -rf "$obj"' EXIT
flags=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function ${XHIST_BUILD_FLAGS:-})
pids=()
tus=(xhist_hot xhist_capi xhist_pick_f64 xhist_pick_f32 xhist_pick_mixed xhist_pick_flat xhist_route_f64_b1024 xhist_route_f64_b1024s8 xhist_route_f32_b1024 xhist_route_f32_b1024s8 xhist_exchange xhist_extrema xhist_meanvar xhist_meanvar_w xhist_quantile xhist_quantile_w xhist_cov xhist_cov_w xhist_map xhist_sum xhist_group xhist_sort xhist_rank)
for tu in "${tus[@]}"; do
  "$HIPCC" "${flags[@]}" -c -o "$obj/$tu.o" "$here/$tu.hip" &
  pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
objs=()
for tu in "${tus[@]}"; do objs+=("$obj/$tu.o"); done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$out.tmp" "${objs[@]}"
mv -f "$out.tmp" "$out"
echo "built $out"
