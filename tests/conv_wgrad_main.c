/* conv_wgrad_main.c -- stand-alone driver of the weight-gradient twin (conv_wgrad_twin.c) and of the host-side repacking of the data
 * gradient's layer (conv_bwd_pack.h): fixed pseudo-random cases, every result printed as hexadecimal words.  The tests build it once
 * plainly and once with -fsanitize=address,undefined; the two must print the same bytes. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_bwd_pack.h"

int conv_wgrad_twin_strips(int B, int H, int cout, int cin, int ks, int s0, int* rows);
void conv_wgrad_twin(const float* g, const float* x, int B, int H, int W, int cout, int cin, int ks, int strips, int rows, float* dw);

static uint32_t rng_state = 12345u;
static float rnd(void)          /* uniform in [-1, 1), exactly representable steps */
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
    /* B, H, W, cout, cin, ks, requested strips: odd sizes, a map smaller than the kernel, strips that end inside an image */
    static const int cases[][7] = {{1, 3, 2, 3, 2, 7, 1}, {2, 5, 3, 4, 3, 3, 3}, {3, 4, 5, 2, 5, 1, 32}, {2, 3, 3, 3, 3, 3, 4}, {1, 1, 1, 1, 1, 7, 5}, {2, 4, 2, 2, 2, 3, 0}};
    for (size_t k = 0; k < sizeof cases / sizeof cases[0]; ++k) {
        const int B = cases[k][0], H = cases[k][1], W = cases[k][2], cout = cases[k][3], cin = cases[k][4], ks = cases[k][5];
        const size_t ng = (size_t)B * cout * H * W, nx = (size_t)B * cin * H * W, nw = (size_t)cout * cin * ks * ks;
        float* g = (float*)malloc(ng * 4);
        float* x = (float*)malloc(nx * 4);
        float* dw = (float*)malloc(nw * 4);
        float* wt = (float*)malloc(nw * 4);
        if (!g || !x || !dw || !wt) return 2;
        for (size_t i = 0; i < ng; ++i) g[i] = rnd();
        for (size_t i = 0; i < nx; ++i) x[i] = rnd();
        int rows = 0;
        const int strips = conv_wgrad_twin_strips(B, H, cout, cin, ks, cases[k][6], &rows);
        printf("case %zu strips %d rows %d\n", k, strips, rows);
        conv_wgrad_twin(g, x, B, H, W, cout, cin, ks, strips, rows, dw);
        dump("dw", dw, nw);
        pmx_conv_flip_weights(dw, cout, cin, ks, wt);
        dump("wt", wt, nw);
        free(g); free(x); free(dw); free(wt);
    }
    return 0;
}
