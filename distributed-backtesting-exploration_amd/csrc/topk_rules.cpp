// topk_rules.cpp — the rules of topk_rules.h. Plain C++: no HIP call, builds with any host compiler.
#include "topk_rules.h"

namespace bt {

std::string sym_id_refusal(int64_t n, const int64_t* ids) {
    for (int64_t s = 0; s < n; ++s)
        if (ids[s] < 0 || ids[s] >= kSymIdEnd)
            return "sym_ids[" + std::to_string(s) + "] = " + std::to_string(ids[s]) + " outside [0, 2^31)";
    return "";
}

std::string topk_of_refusal(int64_t S, int64_t P, int64_t k, bool have_sum, const int32_t* ids, bool have_out) {
    if (S < 1) return "S = " + std::to_string(S) + " is below 1";
    if (P < 1) return "P = " + std::to_string(P) + " is below 1";
    if (S > kTopkOfMax || P > kTopkOfMax || S * P > kTopkOfMax)
        return "S*P = " + std::to_string(S) + "*" + std::to_string(P) + " exceeds 2^22 records";
    if (k < 1 || k > kTopkOfMaxK) return "k = " + std::to_string(k) + " outside [1, " + std::to_string(kTopkOfMaxK) + "]";
    if (!have_sum || !ids || !have_out) return "sum, sym_ids and out are required";
    for (int64_t s = 0; s < S; ++s)
        if (ids[s] < 0) return "sym_ids[" + std::to_string(s) + "] = " + std::to_string(ids[s]) + " is negative";
    return "";
}

}  // namespace bt
