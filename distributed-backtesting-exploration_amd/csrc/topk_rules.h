// topk_rules.h — the pure rules around the top-k order: what bt_topk_of refuses and the range a
// symbol id must lie in. No HIP type: topk_rules.cpp builds with a plain host compiler.
#pragma once
#include <stdint.h>

#include <string>

namespace bt {

constexpr int64_t kTopkOfMax = 1LL << 22;  // records bt_topk_of stages
constexpr int64_t kTopkOfMaxK = 1024;      // kTopkMax of internal.h (analysis.cpp asserts it)
constexpr int64_t kSymIdEnd = 1LL << 31;   // symbol ids lie in [0, kSymIdEnd)

// The id rule: every symbol id of a dataset lies in [0, 2^31). There the device's
// unsigned tie-break word (k_topk.hip sym_param) and the host's signed compare (internal.h
// topk_less) are the same order, and the int32 the engine keeps is the id itself. Returns "" or
// the first offender by index and value.
std::string sym_id_refusal(int64_t n, const int64_t* ids);

// Why bt_topk_of refuses an S x P matrix ("" = accepted), first rule that fails: the shape, the
// staging bound, k, the buffers, then the ids (int32 here, so only a negative one can offend).
std::string topk_of_refusal(int64_t S, int64_t P, int64_t k, bool have_sum, const int32_t* ids, bool have_out);

}  // namespace bt
