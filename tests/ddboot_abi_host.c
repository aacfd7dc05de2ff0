/* ddboot_abi_host — the record of bt_drawdown_boot (include/bt.h) as a compiled C99 host sees it:
 * its size and the offset of every field as one JSON line, under the names of the Python mirror
 * (ddrisk.py DD_RECORDS: a bt_wide field f as f_lo and f_hi), and the limits of the call. Built by
 * tests/test_ddboot_cpu.py with -std=c99 -pedantic -Werror; needs no library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "bt.h"

#define OFF(T, f) printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define WIDE(T, f) printf("\"%s.%s_lo\": %zu, \"%s.%s_hi\": %zu, ", #T, #f, offsetof(T, f.lo), #T, #f, offsetof(T, f.hi))
#define SZ(T) printf("\"%s\": %zu, ", #T, sizeof(T))

int main(void) {
    printf("{");
    SZ(bt_dd_lane); OFF(bt_dd_lane, sum); OFF(bt_dd_lane, mdd); OFF(bt_dd_lane, n_ge); OFF(bt_dd_lane, min_star);
    OFF(bt_dd_lane, max_star); WIDE(bt_dd_lane, m1); WIDE(bt_dd_lane, m2);
    printf("\"levels_max\": %d, \"limits_max\": %d, \"lanes_max\": %d, \"resamples_max\": %d, ", BT_DD_LEVELS_MAX,
           BT_DD_LIMITS_MAX, BT_BOOT_MAX, BT_BOOT_MAX_RESAMPLES);
    printf("\"abi_version\": %d}\n", BT_ABI_VERSION);
    return 0;
}
