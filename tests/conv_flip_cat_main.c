/* conv_flip_cat_main.c -- stand-alone driver of conv_bwd_pack.h::pmx_conv_flip_weights_mapped: the layer whose forward is the data
 * gradient of a 185-input layer (Mconv1_*), with its output channels in the concat buffer's order.  Fixed pseudo-random weights; the map,
 * the weights and the result are printed (the floats as hexadecimal words).  The tests build it once plainly and once with
 * -fsanitize=address,undefined; the two must print the same bytes. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_bwd_pack.h"

/* the concat buffer (csrc/pmx_common.h): [feature 0..127 | PAF 128..165 | pad | heat 168..186 | pad to 192]; the reference's
 * F.concat((h1, h2, feature_map)): 38 PAF, 19 heat, 128 feature */
enum { CAT_C = 192, CAT_FEAT = 0, CAT_PAF = 128, CAT_HEAT = 168, REF_C = 185 };

static uint32_t rng_state = 2468u;
static float rnd(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(int32_t)(rng_state >> 8 & 0xFFFF) / 32768.f - 1.f;
}
static void dump(const char* what, const float* v, size_t n)
{
    printf("%s", what);
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        memcpy(&u, v + i, 4);
        printf(" %08x", u);
    }
    printf("\n");
}

int main(void)
{
    int map[CAT_C];
    for (int k = 0; k < CAT_C; ++k) map[k] = -1;
    for (int i = 0; i < 128; ++i) map[CAT_FEAT + i] = 57 + i;
    for (int i = 0; i < 38; ++i) map[CAT_PAF + i] = i;
    for (int i = 0; i < 19; ++i) map[CAT_HEAT + i] = 38 + i;
    printf("map");
    for (int k = 0; k < CAT_C; ++k) printf(" %d", map[k]);
    printf("\n");
    static const int cases[][2] = {{2, 3}, {1, 7}, {3, 1}};          /* cout, ks */
    for (size_t c = 0; c < sizeof cases / sizeof cases[0]; ++c) {
        const int cout = cases[c][0], ks = cases[c][1];
        const size_t nw = (size_t)cout * REF_C * ks * ks, nt = (size_t)CAT_C * cout * ks * ks;
        float* w = (float*)malloc(nw * 4);
        float* wt = (float*)malloc(nt * 4);
        if (!w || !wt) return 2;
        for (size_t i = 0; i < nw; ++i) w[i] = rnd();
        memset(wt, 0xFF, nt * 4);
        pmx_conv_flip_weights_mapped(w, cout, REF_C, ks, map, CAT_C, wt);
        printf("case %zu cout %d ks %d\n", c, cout, ks);
        dump("w", w, nw);
        dump("wt", wt, nt);
        free(w); free(wt);
    }
    return 0;
}
