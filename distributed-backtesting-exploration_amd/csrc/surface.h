// surface.h — host side of the run reductions (docs/surface_spec.md): what surface.cpp shares with
// analysis.cpp. No HIP type: surface.cpp builds with a plain host compiler (tests/asan).
#pragma once
#include <stdint.h>

#include <string>

#include "host_common.h"

static_assert(sizeof(bt_param_agg) == 104, "bt_param_agg layout");

namespace bt {

constexpr int64_t kSurfaceOfMax = 1LL << 22;       // records bt_surface_of stages
constexpr uint64_t kSurfaceMaxRows = 1ULL << 32;   // dataset rows the int64 sums stay exact below

// Why a reduction of an S x P matrix is refused ("" = accepted): the shape, the outputs, the
// staging bound of bt_surface_of (`bounded`) and the overflow domain of the int64 sums
// (`total_rows`: bars of the resident dataset, 0 when the caller's matrix carries none).
std::string surface_refusal(int64_t S, int64_t P, bool have_out, bool bounded, uint64_t total_rows);

}  // namespace bt
