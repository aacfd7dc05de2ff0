/* tail_abi_host — the two records of bt_tail (include/bt.h) as a compiled C99 host sees them: sizes
 * and the offset of every field as one JSON line, under the names of the Python mirror (tail.py
 * TAIL_RECORDS: a bt_wide field f as f_lo and f_hi), and the limits of the call. Built by
 * tests/test_tail_cpu.py with -std=c99 -pedantic -Werror; needs no library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "bt.h"

#define OFF(T, f) printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define WIDE(T, f) printf("\"%s.%s_lo\": %zu, \"%s.%s_hi\": %zu, ", #T, #f, offsetof(T, f.lo), #T, #f, offsetof(T, f.hi))
#define SZ(T) printf("\"%s\": %zu, ", #T, sizeof(T))

int main(void) {
    printf("{");
    SZ(bt_tail_rec); OFF(bt_tail_rec, n); OFF(bt_tail_rec, n_window); OFF(bt_tail_rec, n_pos); OFF(bt_tail_rec, n_neg);
    OFF(bt_tail_rec, min_bar); OFF(bt_tail_rec, max_bar); OFF(bt_tail_rec, min_d); OFF(bt_tail_rec, max_d);
    OFF(bt_tail_rec, s1); OFF(bt_tail_rec, s1_neg); WIDE(bt_tail_rec, s2); WIDE(bt_tail_rec, s2_neg);
    WIDE(bt_tail_rec, s3); OFF(bt_tail_rec, s4);
    SZ(bt_tail_q); OFF(bt_tail_q, var); OFF(bt_tail_q, es_sum); OFF(bt_tail_q, k); OFF(bt_tail_q, n_lt);
    printf("\"s4_bytes\": %zu, \"tail_max\": %d, \"levels_max\": %d, \"ppm_max\": %d, \"bars_max\": %d, "
           "\"all\": %d, \"held\": %d, ", sizeof(((bt_tail_rec*)0)->s4), BT_TAIL_MAX, BT_TAIL_LEVELS_MAX,
           BT_TAIL_PPM_MAX, BT_TAIL_BARS_MAX, BT_TAIL_ALL, BT_TAIL_HELD);
    printf("\"abi_version\": %d}\n", BT_ABI_VERSION);
    return 0;
}
