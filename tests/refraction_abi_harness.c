/* refraction_abi_harness.c -- TEST-ONLY: the refracted visibility declarations as a C99 compiler reads them from include/topo_hip.h,
 * and their error contract.  Without an argument: what needs no GPU (tests/test_refraction_cpu.py) -- topo_refraction_lift's refusal
 * of k = NaN, -0.01, 1.0 and of a null pointer, and the calls' refusal of a null context.  With the argument `gpu`
 * (tests/test_refraction_gpu.py): on a context without tiles, the read's refusal of the same three k and of 65 observers, and its
 * acceptance of k = 0 and k = TOPO_REFRACTION_STANDARD. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "topo_hip.h"

int main(int argc, char** argv) {
    const double O[3] = {6371100.0, 0.0, 0.0}, P[3] = {6371000.0, 50000.0, 0.0};
    double out[3] = {0.0, 0.0, 0.0}, ll[2] = {7.5, 46.5};
    uint8_t cls[65];
    topo_observer obs[65];
    int i;
    memset(obs, 0, sizeof obs);
    for (i = 0; i < 65; ++i) { obs[i].lon_deg = 7.5; obs[i].lat_deg = 46.5; obs[i].height_m = 10.0; }
    printf("%g\n", TOPO_REFRACTION_STANDARD);
    printf("%d %d %d %d %d %d\n", topo_refraction_lift(O, P, NAN, out), topo_refraction_lift(O, P, -0.01, out), topo_refraction_lift(O, P, 1.0, out),
           topo_refraction_lift(O, P, 0.13, NULL), topo_refraction_lift(O, P, 0.0, out), topo_refraction_lift(O, P, TOPO_REFRACTION_STANDARD, out));
    printf("%d %d %d\n", topo_visibility_refracted_grid_device(NULL, 1, obs, 7.0, 46.0, 0.1, 0.1, 4, 4, 0.0, 0.13, cls, 16, 4),
           topo_visibility_refracted_device(NULL, 1, obs, 1, ll, 0.0, 0.13, cls, 1), topo_visibility_refracted_read(NULL, 1, obs, 1, ll, 0.0, 0.13, cls));
    if (argc > 1 && strcmp(argv[1], "gpu") == 0) {
        topo_ctx* ctx = NULL;
        int rc = topo_create(&ctx, 0, 64, 48, TOPO_FORMAT_RGBA8_UNORM_SRGB);
        if (rc != TOPO_OK) { printf("create %d\n", rc); return 2; }
        printf("%d %d %d %d", topo_visibility_refracted_read(ctx, 1, obs, 1, ll, 0.0, NAN, cls), topo_visibility_refracted_read(ctx, 1, obs, 1, ll, 0.0, -0.01, cls),
               topo_visibility_refracted_read(ctx, 1, obs, 1, ll, 0.0, 1.0, cls), topo_visibility_refracted_read(ctx, 65, obs, 1, ll, 0.0, 0.13, cls));
        memset(cls, 0xAB, sizeof cls);
        printf(" %d", topo_visibility_refracted_read(ctx, 1, obs, 1, ll, 0.0, 0.0, cls));
        printf(" %d %u\n", topo_visibility_refracted_read(ctx, 1, obs, 1, ll, 0.0, TOPO_REFRACTION_STANDARD, cls), (unsigned)cls[0]);
        topo_destroy(ctx);
    }
    /* the lifted point keeps its direction and gains radius */
    if (topo_refraction_lift(O, P, TOPO_REFRACTION_STANDARD, out) != TOPO_OK) return 1;
    return fabs(out[0] / P[0] - out[1] / P[1]) < 1e-12 && out[0] > P[0] && out[2] == 0.0 ? 0 : 1;
}
