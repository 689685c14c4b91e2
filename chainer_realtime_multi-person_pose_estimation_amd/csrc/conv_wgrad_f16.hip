// conv_wgrad_f16.hip -- the weight gradient of a 3x3 / 7x7 layer with f16 operands and fp32 sums (option "grad_precision" = 2 of
// pmx_conv2d_backward; contract: include/pose_mi355x.h, tiling: DESIGN.md 4.7, strip and group rule: wgrad_strips.h).
//
//   GEMM        per tap (ky, kx)  dw[co][ci] = sum over pixels p of f16(g[p][co]) * f16(x[p + (ky-pad, kx-pad)][ci]) on v_mfma_f32_32x32x16_f16:
//               M = co, N = ci, K = 16 pixels per MFMA.  A lane of that MFMA holds EIGHT CONSECUTIVE K of one row / column, i.e. eight pixels
//               of one channel, which NHWC puts ld floats apart -- so both operands go through LDS as [pixel][32 channels] f16 images
//               (64 bytes per pixel) and are read back with the transposed read ds_read_b64_tr_b16: a 16-lane group takes 4 pixels x 16
//               channels and hands each lane its channel's four pixels.  A 32-lane half reads 4 consecutive pixels x 64 bytes = one
//               256-byte bank row: conflict-free at any pixel offset, so a tap shift kx is a 64-byte offset of the same image.
//   groups      every image row is cut into ceil(W / 16) groups of 16 pixels, the last one padded; one MFMA per (group, accumulator).  The
//               g image holds zeros for the pad pixels and the x image zeros for every tap outside the image: pad, don't mask.
//   block       256 threads = (tap row ky, 4 x 32 co: one tile per wave, NCI x 32 ci), NCI = 1 / 2 for 7x7 / 3x3; a wave keeps the KS taps of
//               the row for its NCI ci tiles in NCI x KS accumulators (7 x 16 / 6 x 16 registers), so a g fragment feeds NCI * KS MFMAs.
//               blockIdx.y = the strip of image rows; a step = up to 4 groups (64 pixels) of one image row: 64 x 128 floats of g and
//               (64 + KS - 1) x NCI * 32 floats of x row y + ky - pad, loaded as float4 (a pixel's channels side by side: coalesced),
//               rounded by f16_sat4 (= f16_rn_sat) and written to LDS; the next step's loads are in flight under this step's MFMAs, two
//               buffers, one barrier per step.  Every wave runs every step and every lane every read: the transposed read needs EXEC
//               all ones, so there is no early return and no lane-dependent loop before the epilogue.
//   order       a strip's accumulators go to its slot [strip][tap][co][ci] of the workspace; conv_wgrad_combine_kernel (conv_bwd.hip) adds
//               the slots left to right and writes OIHW.  No atomics.
#include <cstdint>
#include "pmx_ctx.h"
#include "wgrad_strips.h"
#include "f16_sat.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __fp16 h16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 h16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) h16x4 lds_h16x4;

struct WgradF16Args {
    const float* g; const float* x; float* ws;
    int H, W, cg, cx, nco, nci, ncog, rows, groups; // nco / nci: 32-channel tiles of g / x; ncog: sets of 4 co tiles; rows: image rows per strip; groups per image row
    int ldg, ldx;                                   // floats per pixel of g / x (>= cg / cx: the operands may be slices of wider buffers)
    long long total_rows;                           // B * H
};

template <int KS>
struct WgF16 {
    static constexpr int NCI = KS == 7 ? 1 : 2, PAD = KS / 2;
    static constexpr int GP = 4, PIX = 16 * GP, XPIX = PIX + KS - 1;        // groups / pixels of g / pixels of x per step
    static constexpr int ROW = 64;                                         // bytes per pixel of an image: 32 channels f16
    static constexpr int G_IMG = PIX * ROW, X_IMG = XPIX * ROW, BUF = 4 * G_IMG + NCI * X_IMG;      // [4 co tiles of g | NCI ci tiles of x]
    static constexpr int NGF = PIX * 32 / 256;                             // float4 per thread of the g tile (128 channels per pixel)
    static constexpr int X_UNITS = XPIX * NCI * 8, NXF = (X_UNITS + 255) / 256;
    static_assert(BUF % 16 == 0 && G_IMG % 16 == 0 && X_IMG % 16 == 0, "LDS images are 16-byte aligned");
};

// the two transposed reads of a 32x32x16 operand: pixels 8h + 0..3 and 8h + 4..7 of this lane's channel
__device__ __forceinline__ f16x8 tr_operand(const char* p)
{
    const h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h16x4*)p);
    const h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h16x4*)(p + 4 * 64));
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int KS>
__global__ void __launch_bounds__(256) conv_wgrad_f16_kernel(WgradF16Args a)
{
    using C = WgF16<KS>;
    constexpr int NCI = C::NCI, PAD = C::PAD;
    extern __shared__ float4 smem4[];               // (no static LDS in front of it: the base is 16-byte aligned)
    char* const lds = reinterpret_cast<char*>(smem4);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cog = blockIdx.x % a.ncog, ky = (blockIdx.x / a.ncog) % KS, cig = blockIdx.x / (a.ncog * KS);
    const int co_t = cog * 4 + wave;
    const long long r0 = (long long)blockIdx.y * a.rows;
    const long long r1 = r0 + a.rows < a.total_rows ? r0 + a.rows : a.total_rows;
    const int H = a.H, W = a.W;
    const int groups = a.groups, chunks = (groups + C::GP - 1) / C::GP;
    const long long nsteps = (r1 - r0) * chunks;    // (>= 1: the launch checks that every strip has a row)

    // staging: g unit r = (pixel (tid >> 5) + 8 r, channels 4 c4 .. 4 c4 + 3 of the block's 128), x unit f = tid + 256 r = (pixel, 4 channels)
    const int g_c4 = tid & 31, g_ch = cog * 128 + 4 * g_c4;
    const bool g_cok = g_ch < a.cg;
    const int g_lds = (g_c4 >> 3) * C::G_IMG + (tid >> 5) * C::ROW + (g_c4 & 7) * 8;
    int x_pix[C::NXF], x_ch[C::NXF], x_lds[C::NXF];
#pragma unroll
    for (int r = 0; r < C::NXF; ++r) {
        const int f = tid + 256 * r, c4 = f % (NCI * 8);
        const bool slot = f < C::X_UNITS;
        x_pix[r] = slot ? f / (NCI * 8) : -1;
        x_ch[r] = cig * NCI * 32 + 4 * c4;
        x_lds[r] = 4 * C::G_IMG + (c4 >> 3) * C::X_IMG + (f / (NCI * 8)) * C::ROW + (c4 & 7) * 8;
    }
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // Every lane always loads: one without an operand (pad pixel, tap outside the image, channel tile past the layer's last) reads the
    // first four floats of the buffer, which are in bounds, and the value is replaced by zeros -- no branch per load.
    // the step to load next: image row `row` of the batch's B * H (row y of its image), pixels [64 ch, 64 ch + 64) of it
    long long row = r0;
    int y = (int)(r0 % H), ch = 0;
    auto load = [&](float4 (&gv)[C::NGF], float4 (&xv)[C::NXF]) {
        const int xs0 = ch * C::PIX, yy = y + ky - PAD;
        const float* gp = a.g + (size_t)row * W * a.ldg + g_ch;
#pragma unroll
        for (int r = 0; r < C::NGF; ++r) {
            const int col = xs0 + (tid >> 5) + 8 * r;
            const bool ok = g_cok && col < W;
            const float4 v = *reinterpret_cast<const float4*>(ok ? gp + (size_t)col * a.ldg : a.g);
            gv[r] = ok ? v : zero4;
        }
        const bool yok = (unsigned)yy < (unsigned)H;
        const float* xp = a.x + (size_t)(yok ? row + ky - PAD : row) * W * a.ldx;
#pragma unroll
        for (int r = 0; r < C::NXF; ++r) {
            const int col = xs0 - PAD + x_pix[r];
            const bool ok = yok && x_pix[r] >= 0 && (unsigned)col < (unsigned)W && x_ch[r] < a.cx;
            const float4 v = *reinterpret_cast<const float4*>(ok ? xp + (size_t)col * a.ldx + x_ch[r] : a.x);
            xv[r] = ok ? v : zero4;
        }
        if (++ch == chunks) { ch = 0; ++row; y = y + 1 == H ? 0 : y + 1; }
    };
    auto store = [&](char* buf, const float4 (&gv)[C::NGF], const float4 (&xv)[C::NXF]) {
#pragma unroll
        for (int r = 0; r < C::NGF; ++r) *reinterpret_cast<f16x4*>(buf + g_lds + 8 * r * C::ROW) = f16_sat4(gv[r]);
#pragma unroll
        for (int r = 0; r < C::NXF; ++r)
            if (x_pix[r] >= 0) *reinterpret_cast<f16x4*>(buf + x_lds[r]) = f16_sat4(xv[r]);
    };

    f32x16 acc[NCI][KS];
#pragma unroll
    for (int j = 0; j < NCI; ++j)
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][k][e] = 0.f;

    // this lane's address inside a 16-pixel group of an image: lane 4q + p of a 16-lane group supplies pixel q, channels 4p .. 4p + 3 of the
    // group's 16 channels; groups 0 / 1 are channels 0-15 / 16-31 of K half 0 (pixels 0-7), groups 2 / 3 those of K half 1 (pixels 8-15)
    const int frag = (8 * (lane >> 5) + ((lane & 15) >> 2)) * C::ROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    const int a_off = wave * C::G_IMG + frag, b_off = 4 * C::G_IMG + frag;

    {
        float4 gv[C::NGF], xv[C::NXF];
        load(gv, xv);
        store(lds, gv, xv);
    }
    __syncthreads();
    int left = groups;                              // groups of the current image row not yet multiplied
    for (long long s = 0; s < nsteps; ++s) {
        const char* cur = lds + (s & 1) * C::BUF;
        char* nxt = lds + ((s + 1) & 1) * C::BUF;
        const bool more = s + 1 < nsteps;
        float4 gn[C::NGF], xn[C::NXF];
        if (more) load(gn, xn);             // the next step: global -> registers under this step's MFMAs
        const int ng = left < C::GP ? left : C::GP;
        left = left > C::GP ? left - C::GP : groups;
        if (co_t < a.nco) {                         // (wave-uniform: a wave without a co tile skips the MFMAs, not the barriers)
            for (int gi = 0; gi < ng; ++gi) {
                const f16x8 av = tr_operand(cur + a_off + gi * 16 * C::ROW);
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int j = 0; j < NCI; ++j) {
                        const f16x8 bv = tr_operand(cur + b_off + j * C::X_IMG + (gi * 16 + kx) * C::ROW);
                        acc[j][kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc[j][kx], 0, 0, 0);
                    }
            }
        }
        if (more) {
            store(nxt, gn, xn);                     // (the other buffer: its last readers passed the previous barrier)
            __syncthreads();
        }
    }

    // D[i][j]: i = co (the A rows), j = ci (the B columns); lane: j = l, i = (e & 3) + 8 * (e >> 2) + 4 * half
    if (co_t >= a.nco) return;
    const int l = lane & 31, half = lane >> 5;
    const size_t tile = (size_t)a.cg * a.cx;
#pragma unroll
    for (int j = 0; j < NCI; ++j) {
        if (cig * NCI + j >= a.nci) continue;       // (a ci tile past the layer's last multiplied zeros)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            float* o = a.ws + ((size_t)blockIdx.y * (KS * KS) + ky * KS + kx) * tile + (size_t)(co_t * 32) * a.cx + (cig * NCI + j) * 32 + l;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[(size_t)((e & 3) + 8 * (e >> 2) + 4 * half) * a.cx] = acc[j][kx][e];
        }
    }
}

template <int KS>
void launch_wgrad_f16(const WgradF16Args& a, int strips, hipStream_t stream)
{
    const dim3 grid((unsigned)pmx_wgrad_f16_blocks(a.cg, a.cx, KS), (unsigned)strips);
    hipLaunchKernelGGL((conv_wgrad_f16_kernel<KS>), grid, dim3(256), 2 * WgF16<KS>::BUF, stream, a);
}

}  // namespace

int conv_wgrad_f16_strips(int B, int H, int cg, int cx, int ks, int forced, int* rows)
{
    return pmx_wgrad_f16_strips(B, H, cg, cx, ks, forced, PMX_WGRAD_MAX_STRIPS, rows);
}

int conv_wgrad_f16_launch(const float* g, int ldg, const float* x, int ldx, float* ws, float* dw, int B, int H, int W, int cout, int cg, int cin, int cx,
                          int ks, int strips, int rows, const int* cin_map, hipStream_t stream, int max_strips)
{
    const long long total = (long long)B * H;
    PMX_CHECK(g && x && ws && dw && B >= 1 && H >= 1 && W >= 1, PMX_ERR_INVALID, "conv_wgrad_f16: bad arguments");
    PMX_CHECK(cg % 32 == 0 && cx % 32 == 0 && cg >= cout && cx >= cin && cout >= 1 && cin >= 1 && ldg >= cg && ldx >= cx && (ks == 3 || ks == 7),
              PMX_ERR_INVALID, "conv_wgrad_f16: bad channels / ksize");
    PMX_CHECK(ldg % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)x & 15) == 0, PMX_ERR_INVALID,
              "conv_wgrad_f16: the operands are read 16 bytes at a time");
    PMX_CHECK(rows >= 1 && strips >= 1 && strips <= max_strips && (long long)(strips - 1) * rows < total && (long long)strips * rows >= total,
              PMX_ERR_INVALID, "conv_wgrad_f16: %d strips of %d rows do not cover %lld rows", strips, rows, total);
    WgradF16Args a;
    a.g = g; a.x = x; a.ws = ws; a.H = H; a.W = W; a.cg = cg; a.cx = cx; a.nco = cg / 32; a.nci = cx / 32; a.ncog = (a.nco + 3) / 4;
    a.rows = rows; a.groups = pmx_wgrad_f16_groups(W); a.ldg = ldg; a.ldx = ldx; a.total_rows = total;
    if (ks == 7) launch_wgrad_f16<7>(a, strips, stream);
    else launch_wgrad_f16<3>(a, strips, stream);
    PMX_HIP(hipGetLastError());
    return conv_wgrad_combine_launch(ws, dw, strips, ks, cout, cin, cg, cx, cin_map, stream);
}
