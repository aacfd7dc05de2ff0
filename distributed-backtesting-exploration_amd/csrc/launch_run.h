// launch_run.h — the launches of one strategy run, shared by launch_sma, launch_ema_ols and
// launch_boll: what the LaunchPlan (plan.h) says, in one place.
#pragma once
#include <type_traits>

#include "internal.h"
#include "plan.h"

namespace bt {

enum class Variant { kPlain, kParity, kSeg };
template <Variant V>
using VariantTag = std::integral_constant<Variant, V>;

// Enqueues a fold kernel (*_seg_combine) over a split run's records: one lane per (symbol, param),
// 256 per block.
template <class Rec>
void enqueue_fold(void (*kernel)(const SymDesc*, int, int, const Rec*, int, double, Out), const void* rec,
                  const SymDesc* syms, int32_t n_sym, const Grid& g, int G, const Out& out, hipStream_t st) {
    const size_t n = (size_t)n_sym * g.n_params;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, syms, n_sym, g.n_params,
                       static_cast<const Rec*>(rec), G, g.sqrt_ann, out);
}

// `kernel(variant tag, grid, s)` enqueues the strategy's kernel, `fold()` its segment fold
// (*_seg_combine). A split run (G > 1) is the speculative segments (blockIdx.z = segment), then the
// fix pass of each boundary s in order (a block returns at once when its lanes' starts were
// right), then the fold; an unsplit run (G == 1) is the parity or the plain kernel.
template <class K, class F>
hipError_t launch_run(const K& kernel, const F& fold, int32_t n_sym, bool parity, const LaunchPlan& pl) {
    const dim3 grid(n_sym, pl.grid_y, pl.G), fgrid(n_sym, pl.grid_y, 1);
    if (pl.G > 1) {
        kernel(VariantTag<Variant::kSeg>{}, grid, 0);
        for (int s = 1; s < pl.G; ++s) kernel(VariantTag<Variant::kSeg>{}, fgrid, s);
        fold();
    } else if (parity) {
        kernel(VariantTag<Variant::kParity>{}, grid, 0);
    } else {
        kernel(VariantTag<Variant::kPlain>{}, grid, 0);
    }
    return hipGetLastError();
}

}  // namespace bt
