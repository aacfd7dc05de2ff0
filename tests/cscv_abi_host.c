/* cscv_abi_host — the two records of bt_cscv (include/bt.h) as a compiled C99 host sees them: sizes
 * and the offset of every field as one JSON line, under the names of the Python mirror
 * (overfit.py CSCV_RECORDS). Built by tests/test_cscv_cpu.py with -std=c99 -pedantic -Werror; needs
 * no library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "bt.h"

#define OFF(T, f) printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define SZ(T) printf("\"%s\": %zu, ", #T, sizeof(T))

int main(void) {
    printf("{");
    SZ(bt_cscv_group); OFF(bt_cscv_group, sym); OFF(bt_cscv_group, n_lanes); OFF(bt_cscv_group, n_live);
    OFF(bt_cscv_group, n_dead); OFF(bt_cscv_group, n_overfit); OFF(bt_cscv_group, n_loss);
    OFF(bt_cscv_group, n_tied); OFF(bt_cscv_group, pad);
    SZ(bt_cscv_pick); OFF(bt_cscv_pick, lane); OFF(bt_cscv_pick, r2); OFF(bt_cscv_pick, is_sharpe);
    OFF(bt_cscv_pick, oos_sharpe);
    printf("\"abi_version\": %d}\n", BT_ABI_VERSION);
    return 0;
}
