/* summits_abi_harness.c -- TEST-ONLY: the summit calls' structs and constants as a C99 compiler lays them out from include/topo_hip.h
 * (tests/test_summits_cpu.py compares them with the ctypes binding's).  Calls nothing: it needs no library. */
#include <stddef.h>
#include <stdio.h>

#include "topo_hip.h"

int main(void) {
    printf("%zu %zu %zu\n", sizeof(topo_summit_params), sizeof(topo_summit), sizeof(topo_summit_snap));
    printf("%u %u %u\n", TOPO_SUMMIT_ORDER_TILE, TOPO_SUMMIT_ORDER_HEIGHT, TOPO_SUMMIT_ORDER_ISOLATION);
    printf("%d %d %d\n", TOPO_SNAP_FOUND, TOPO_SNAP_NONE, TOPO_SNAP_INVALID);
    return offsetof(topo_summit, higher_vy) == 60 && offsetof(topo_summit_snap, vy) == 44 && offsetof(topo_summit_params, order) == 20 ? 0 : 1;
}
