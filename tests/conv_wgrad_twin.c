/* conv_wgrad_twin.c -- the order-defined host twin of the weight-gradient kernel (csrc/conv_bwd.hip): the summation order that
 * include/pose_mi355x.h::pmx_conv2d_backward documents, with fmaf.  Built by the tests with the host compiler and -ffp-contract=off.
 *
 * g: (B, cout, H, W), x: (B, cin, H, W), dw: (cout, cin, ks, ks), all float32 NCHW / OIHW.  The B * H image rows are cut into `strips`
 * strips of `rows` consecutive rows (the last one may be shorter); conv_wgrad_twin_strips gives the library's (strips, rows) for a
 * requested count s0 (option "wgrad_strips"; 0 = the automatic count: 2048 waves over the layer's units of one tap row x 32 co x
 * 32 / 64 / 128 ci for 7x7 / 3x3 / 1x1). */
#include <math.h>
#include <stddef.h>

int conv_wgrad_twin_strips(int B, int H, int cout, int cin, int ks, int s0, int* rows)
{
    const long long total = (long long)B * H;
    long long s = s0;
    if (s <= 0) {
        const int per = ks == 7 ? 1 : ks == 3 ? 2 : 4, nci = (cin + 31) / 32, nco = (cout + 31) / 32;
        const long long units = (long long)((nci + per - 1) / per) * ks * nco;
        s = (2048 + units - 1) / units;
    }
    if (s > 32) s = 32;                 /* PMX_WGRAD_MAX_STRIPS */
    if (s > total) s = total;
    if (s < 1) s = 1;
    const long long r = (total + s - 1) / s;
    *rows = (int)r;
    return (int)((total + r - 1) / r);
}

void conv_wgrad_twin(const float* g, const float* x, int B, int H, int W, int cout, int cin, int ks, int strips, int rows, float* dw)
{
    const int pad = ks / 2;
    const long long total = (long long)B * H;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) {
                    float sum = 0.f;
                    for (int s = 0; s < strips; ++s) {
                        const long long r0 = (long long)s * rows, r1 = r0 + rows < total ? r0 + rows : total;
                        float acc = 0.f;
                        for (long long r = r0; r < r1; ++r) {
                            const int n = (int)(r / H), y = (int)(r % H), yy = y + ky - pad;
                            const float* grow = g + (((size_t)n * cout + co) * H + y) * W;
                            const float* xrow = x + (((size_t)n * cin + ci) * H + (yy >= 0 && yy < H ? yy : 0)) * W;
                            for (int xx = 0; xx < W; ++xx) {
                                const int sx = xx + kx - pad;
                                const float xv = yy >= 0 && yy < H && sx >= 0 && sx < W ? xrow[sx] : 0.f;
                                acc = fmaf(grow[xx], xv, acc);
                            }
                        }
                        if (((r1 - r0) * W) & 1) acc = fmaf(0.f, 0.f, acc);        /* the MFMA's second K slot of the last pixel pair */
                        sum = s == 0 ? acc : sum + acc;
                    }
                    dw[(((size_t)co * cin + ci) * ks + ky) * ks + kx] = sum;
                }
}
