// surface_plan_driver — prints what bt_surface would launch for an S x P matrix, without a GPU:
// the SurfacePlan of csrc/plan.cpp as one JSON line, with every chunk's rows spelled out and the
// staging layout (staged = 1: with the matrix and ids bt_surface_of uploads).
//
//   surface_plan_driver S P cus chunks_req [staged]
#include <cstdio>
#include <cstdlib>

#include "plan.h"

using namespace bt;

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) return 2;
    const int32_t S = atoi(argv[1]), P = atoi(argv[2]), cus = atoi(argv[3]), req = atoi(argv[4]);
    const SurfacePlan pl = plan_surface(S, P, cus, req, argc == 6 && atoi(argv[5]) != 0);
    printf("{\"block\": %d, \"p_blocks\": %d, \"chunks\": %d, \"rows_per_chunk\": %d, \"rows_rem\": %d, "
           "\"p_tiles\": %d, \"fold_ways\": %d, \"fold_bytes\": %zu, \"partial_bytes\": %zu, \"best_partial_bytes\": %zu, \"agg_bytes\": %zu, "
           "\"o_partial\": %zu, \"o_fold\": %zu, \"o_best_partial\": %zu, \"o_agg\": %zu, \"o_best\": %zu, \"o_sum\": %zu, "
           "\"o_ids\": %zu, \"staging_bytes\": %zu, \"rows\": [",
           pl.block, pl.p_blocks, pl.chunks, pl.rows_per_chunk, pl.rows_rem, pl.p_tiles, pl.fold_ways,
           pl.fold_bytes, pl.partial_bytes,
           pl.best_partial_bytes, sizeof(bt_param_agg), pl.o_partial, pl.o_fold, pl.o_best_partial, pl.o_agg,
           pl.o_best, pl.o_sum, pl.o_ids, pl.staging_bytes);
    // the rows of chunk c exactly as k_surface.hip surface_pass computes them
    for (int32_t c = 0; c < pl.chunks; ++c) {
        const int32_t r0 = c * pl.rows_per_chunk + (c < pl.rows_rem ? c : pl.rows_rem);
        const int32_t r1 = r0 + pl.rows_per_chunk + (c < pl.rows_rem ? 1 : 0);
        printf("%s[%d, %d]", c ? ", " : "", r0, r1);
    }
    printf("]}\n");
    return 0;
}
