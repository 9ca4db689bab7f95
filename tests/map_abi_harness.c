/* map_abi_harness.c -- TEST-ONLY: the map calls' struct and constants as a C99 compiler lays them out from include/topo_hip.h
 * (tests/test_map_cpu.py compares them with the ctypes binding's), and the entry points that need no GPU: topo_map_xy, and the
 * refusal of a null context. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "topo_hip.h"

int main(void) {
    topo_map_params p;
    double ll[4] = {10.5, 46.25, 0.0, 91.0}, xy[4] = {0, 0, 0, 0};
    memset(&p, 0, sizeof p);
    p.lon0_deg = 10.0; p.lat0_deg = 47.0; p.dlon_deg = 0.25; p.dlat_deg = -0.25; p.nx = 8; p.ny = 8;
    topo_map_xy(&p, 2, ll, xy);
    printf("%zu %zu %zu %zu %zu\n", sizeof(topo_map_params), offsetof(topo_map_params, nx), offsetof(topo_map_params, sun_direction), offsetof(topo_map_params, void_rgba),
           offsetof(topo_map_params, reserved));
    printf("%u %u %u %u %u %u %u\n", TOPO_MAP_RELIEF, TOPO_MAP_CONTOURS, TOPO_MAP_SEEN, TOPO_MAP_FLAG_TERRAIN, TOPO_MAP_FLAG_CONTOUR, TOPO_MAP_FLAG_INDEX, TOPO_MAP_FLAG_SEEN);
    printf("%g %g %d %d\n", xy[0], xy[1], isnan(xy[2]) != 0, isnan(xy[3]) != 0);
    printf("%d %d\n", topo_map_device(NULL, &p, NULL, 0, NULL, 0), topo_map_read(NULL, &p, NULL, NULL));
    return xy[0] == 2.0 && xy[1] == 3.0 ? 0 : 1;
}
