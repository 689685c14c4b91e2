// pmx_samples.hip -- validation and training samples on the device: the pixel side of CocoDataLoader.generate_labels
// (coco_data_loader.py:72-205, 334-341) for a whole batch of images of different sizes.
//
//   resize    cv2.resize (linear, uint8) of image and mask per sample: prep.hip::resize_linear_u8_kernel's arithmetic, sizes and tables
//             through a per-sample descriptor.  The mask goes through as 0/1 bytes and is tested != 0 (:77).
//   window    random_rotate_img + random_crop_img + distort_color + flip_img for the insize x insize crop window only: the rotated image
//             as a whole never exists.  Cubic warp of the image, linear warp of the mask x 255, both in the fixed-point scheme of the
//             header; integer BGR->HSV, the three offsets, float32 HSV->BGR; the mirror is the store index.
//   dilation  the 16 x 16 MORPH_DILATE of the insize x insize mask (:340), rows then columns, window -8 .. +7.
// Every kernel is a gather (a destination pixel reads source pixels only): no atomics, the same bits on every run.  One launch per step
// over all samples of the call; the samples' geometry is a device table.  This file is compiled with -ffp-contract=off: the float64
// coordinates and the float32 colour formula are evaluated product by product, as the NumPy restatement (tests/sample_ref.py) does.
#include "pmx_ctx.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int TAB = 32;                  // fractions per pixel
constexpr int W_ONE = 32768;             // weight scale
constexpr size_t N_CUBIC = (size_t)TAB * TAB * 16, N_LINEAR = (size_t)TAB * TAB * 4;

// one sample as the kernels see it.  A = the image the window is cut from or warped from (the resized source, or the source itself)
struct SampleDev {
    const uint8_t* src; const uint8_t* msk;          // source image (sh x sw x 3) and mask (sh x sw) or null
    const uint8_t* a_img; const uint8_t* a_msk;      // train: A and its mask (0/1 bytes; null = no mask)
    uint8_t* rs_img; uint8_t* rs_msk;                // resize destination: A (train) or the sample's output (validation); null = no resize
    const int* xtab; const int* ytab;                // resize tables of (rs_w, rs_h)
    double M[6];                                     // inverse matrix (rotate)
    int sh, sw, rs_h, rs_w, ah, aw;
    int train, rotate, rot_w, rot_h, ox, oy, distort, d[3], flip;
};

// Constants of the contract, built once on the host: [cubic weights int32 32 x 32 x 16 | linear weights int32 32 x 32 x 4 | sdiv int 256 | hdiv int 256]
constexpr size_t CONST_BYTES = (N_CUBIC + N_LINEAR) * sizeof(int32_t) + 512 * sizeof(int);

void fix_sum(int* w, int n)
{
    int sum = 0, big = 0;
    for (int k = 0; k < n; ++k) { sum += w[k]; if (w[k] > w[big]) big = k; }       // first of the largest in row-major order
    w[big] += W_ONE - sum;
}

void build_weights(const float (*co)[4], int n, int32_t* out)
{
    for (int fy = 0; fy < TAB; ++fy)
        for (int fx = 0; fx < TAB; ++fx) {
            int w[16];
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    const float p = co[fy][i] * co[fx][j];
                    w[i * n + j] = (int)lrintf(p * (float)W_ONE);
                }
            fix_sum(w, n * n);
            for (int k = 0; k < n * n; ++k) out[((size_t)fy * TAB + fx) * n * n + k] = (int32_t)w[k];
        }
}

void build_consts(char* host)
{
    float cub[TAB][4], lin[TAB][4];
    const float A = -0.75f;
    for (int f = 0; f < TAB; ++f) {
        const float x = (float)f / (float)TAB, x1 = x + 1.0f, xm = 1.0f - x;
        float c0 = A * x1;  c0 = c0 - 5.0f * A;  c0 = c0 * x1;  c0 = c0 + 8.0f * A;  c0 = c0 * x1;  c0 = c0 - 4.0f * A;
        float c1 = (A + 2.0f) * x;  c1 = c1 - (A + 3.0f);  c1 = c1 * x;  c1 = c1 * x;  c1 = c1 + 1.0f;
        float c2 = (A + 2.0f) * xm;  c2 = c2 - (A + 3.0f);  c2 = c2 * xm;  c2 = c2 * xm;  c2 = c2 + 1.0f;
        float c3 = 1.0f - c0;  c3 = c3 - c1;  c3 = c3 - c2;
        cub[f][0] = c0; cub[f][1] = c1; cub[f][2] = c2; cub[f][3] = c3;
        lin[f][0] = xm; lin[f][1] = x; lin[f][2] = lin[f][3] = 0.f;
    }
    int32_t* wc = (int32_t*)host;
    build_weights(cub, 4, wc);
    build_weights(lin, 2, wc + N_CUBIC);
    int* sdiv = (int*)(wc + N_CUBIC + N_LINEAR);
    int* hdiv = sdiv + 256;
    sdiv[0] = hdiv[0] = 0;
    for (int i = 1; i < 256; ++i) {
        sdiv[i] = (int)lrint(255.0 * 4096.0 / (double)i);
        hdiv[i] = (int)lrint(180.0 * 4096.0 / (6.0 * (double)i));
    }
}

// ---- resize: one thread per destination pixel; blockIdx = (pixels / 256, sample, 0 image | 1 mask) --------------------------------
__global__ void __launch_bounds__(256) samples_resize_kernel(const SampleDev* __restrict__ tab)
{
    const SampleDev& s = tab[blockIdx.y];
    if (!s.rs_img) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.rs_h * s.rs_w) return;
    const int x = i % s.rs_w, y = i / s.rs_w, dw = s.rs_w, dh = s.rs_h;
    const int sx0 = s.xtab[x], sx1 = s.xtab[dw + x], a0 = s.xtab[2 * dw + x], a1 = s.xtab[3 * dw + x];
    const int sy0 = s.ytab[y], sy1 = s.ytab[dh + y], b0 = s.ytab[2 * dh + y], b1 = s.ytab[3 * dh + y];
    if (blockIdx.z == 0) {
        const uint8_t* r0 = s.src + (size_t)sy0 * s.sw * 3;
        const uint8_t* r1 = s.src + (size_t)sy1 * s.sw * 3;
        uint8_t* o = s.rs_img + (size_t)i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int S0 = (int)r0[sx0 * 3 + c] * a0 + (int)r0[sx1 * 3 + c] * a1;
            const int S1 = (int)r1[sx0 * 3 + c] * a0 + (int)r1[sx1 * 3 + c] * a1;
            int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
            o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    } else {
        int v = 0;
        if (s.msk) {
            const uint8_t* r0 = s.msk + (size_t)sy0 * s.sw;
            const uint8_t* r1 = s.msk + (size_t)sy1 * s.sw;
            const int S0 = (r0[sx0] ? 1 : 0) * a0 + (r0[sx1] ? 1 : 0) * a1;
            const int S1 = (r1[sx0] ? 1 : 0) * a0 + (r1[sx1] ? 1 : 0) * a1;
            v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        }
        s.rs_msk[i] = v != 0 ? 1 : 0;
    }
}

// ---- colour ------------------------------------------------------------------------------------------------------------------------
__device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ inline void distort_bgr(int& b, int& g, int& r, const int* d, const int* __restrict__ sdiv, const int* __restrict__ hdiv)
{
    int v = b > g ? b : g; v = v > r ? v : r;
    int mn = b < g ? b : g; mn = mn < r ? mn : r;
    const int diff = v - mn;
    int s = (diff * sdiv[v] + 2048) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + 2048) >> 12;
    if (h < 0) h += 180;
    h = clamp255((int)(uint8_t)h + d[0]);              // the reference clamps the hue, it does not wrap it (:167)
    s = clamp255((int)(uint8_t)s + d[1]);
    v = clamp255(v + d[2]);
    const float vf = (float)v * (float)(1.0 / 255.0);
    float fb = vf, fg = vf, fr = vf;
    if (s != 0) {
        const float sf = (float)s * (float)(1.0 / 255.0);
        float hf = (float)(h % 180) * (float)(6.0 / 180.0);
        const float fl = floorf(hf);
        int sec = (int)fl;
        hf = hf - fl;
        if (sec < 0 || sec >= 6) { sec = 0; hf = 0.f; }
        const float t0 = vf, t1 = vf * (1.0f - sf), t2 = vf * (1.0f - sf * hf), t3 = vf * (1.0f - sf * (1.0f - hf));
        switch (sec) {
            case 0: fb = t1; fg = t3; fr = t0; break;
            case 1: fb = t1; fg = t0; fr = t2; break;
            case 2: fb = t3; fg = t0; fr = t1; break;
            case 3: fb = t0; fg = t2; fr = t1; break;
            case 4: fb = t0; fg = t1; fr = t3; break;
            default: fb = t2; fg = t1; fr = t0; break;
        }
    }
    b = clamp255((int)rintf(fb * 255.0f));
    g = clamp255((int)rintf(fg * 255.0f));
    r = clamp255((int)rintf(fr * 255.0f));
}

// source coordinate of destination (x, y) along one axis, in 1/32 pixel: (rint((Mb * y + Mc) * 1024) + 16 + rint(Ma * x * 1024)) >> 5
__device__ inline long long warp_coord(double Ma, double Mb, double Mc, double x, double y)
{
    return (llrint((Mb * y + Mc) * 1024.0) + 16 + llrint(Ma * x * 1024.0)) >> 5;
}

// ---- window: one thread per pixel of the insize x insize window of a training sample; blockIdx = (pixels / 256, sample) -----------------
__global__ void __launch_bounds__(256) samples_window_kernel(const SampleDev* __restrict__ tab, const int32_t* __restrict__ wcub,
                                                             const int32_t* __restrict__ wlin, const int* __restrict__ sdiv,
                                                             const int* __restrict__ hdiv, uint8_t* __restrict__ out, uint8_t* __restrict__ mask,
                                                             int insize)
{
    const SampleDev& s = tab[blockIdx.y];
    if (!s.train) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= insize * insize) return;
    const int x = i % insize, y = i / insize;
    const int u = x + s.ox, v = y + s.oy;                   // the pixel of the (rotated) image under this window pixel
    int b = 127, g = 127, r = 127, m = 0;                   // crop fill: uint8(127.5), False (:137-138)
    if (u >= 0 && u < s.rot_w && v >= 0 && v < s.rot_h) {
        if (!s.rotate) {
            const uint8_t* p = s.a_img + ((size_t)v * s.aw + u) * 3;
            b = p[0]; g = p[1]; r = p[2];
            m = s.a_msk ? s.a_msk[(size_t)v * s.aw + u] : 0;
        } else {
            const long long X = warp_coord(s.M[0], s.M[1], s.M[2], (double)u, (double)v);
            const long long Y = warp_coord(s.M[3], s.M[4], s.M[5], (double)u, (double)v);
            const long long sx = X >> 5, sy = Y >> 5;
            const int fx = (int)(X & 31), fy = (int)(Y & 31);
            if (sx < -3 || sx > s.aw + 1 || sy < -3 || sy > s.ah + 1) {          // every tap is border: the weights add up to W_ONE exactly
                b = g = r = 128;
            } else {
                const int32_t* w = wcub + ((size_t)fy * TAB + fx) * 16;
                int ab = 0, ag = 0, ar = 0;
                for (int k = 0; k < 4; ++k) {
                    const int yy = (int)sy - 1 + k;
                    for (int j = 0; j < 4; ++j) {
                        const int xx = (int)sx - 1 + j, wt = w[k * 4 + j];
                        int pb = 128, pg = 128, pr = 128;            // border: round-half-even of 127.5
                        if (yy >= 0 && yy < s.ah && xx >= 0 && xx < s.aw) {
                            const uint8_t* p = s.a_img + ((size_t)yy * s.aw + xx) * 3;
                            pb = p[0]; pg = p[1]; pr = p[2];
                        }
                        ab += wt * pb; ag += wt * pg; ar += wt * pr;
                    }
                }
                b = clamp255((ab + 16384) >> 15); g = clamp255((ag + 16384) >> 15); r = clamp255((ar + 16384) >> 15);
                if (s.a_msk) {
                    const int32_t* wl = wlin + ((size_t)fy * TAB + fx) * 4;
                    int am = 0;
                    for (int k = 0; k < 2; ++k) {
                        const int yy = (int)sy + k;
                        for (int j = 0; j < 2; ++j) {
                            const int xx = (int)sx + j;
                            if (yy >= 0 && yy < s.ah && xx >= 0 && xx < s.aw && s.a_msk[(size_t)yy * s.aw + xx]) am += wl[k * 2 + j] * 255;
                        }
                    }
                    m = clamp255((am + 16384) >> 15) > 0 ? 1 : 0;
                }
            }
        }
    }
    if (s.distort) distort_bgr(b, g, r, s.d, sdiv, hdiv);
    const int xo = s.flip ? insize - 1 - x : x;
    const size_t o = ((size_t)blockIdx.y * insize + y) * insize + xo;
    out[o * 3] = (uint8_t)b; out[o * 3 + 1] = (uint8_t)g; out[o * 3 + 2] = (uint8_t)r;
    mask[o] = (uint8_t)m;
}

// ---- dilation: four pixels per thread (insize is a multiple of 8: every row starts 4-byte aligned) --------------------------------
// rows: out[y, x] = max in[y, x-8 .. x+7]; columns: the same along y.  Nothing outside the image contributes.
template <bool ROWS>
__global__ void __launch_bounds__(256) samples_dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n, int insize)
{
    const int q = insize / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * insize * q) return;
    const int x0 = (int)(i % q) * 4;
    const long long row = i / q;                             // sample * insize + y
    const int y = (int)(row % insize);
    const uint8_t* img = in + (row - y) * insize;
    uchar4 o = make_uchar4(0, 0, 0, 0);
    if (ROWS) {
        const uint8_t* r = img + (size_t)y * insize;
        uint8_t t[19];                                         // x0-8 .. x0+10
#pragma unroll
        for (int k = 0; k < 19; ++k) { const int x = x0 - 8 + k; t[k] = (x >= 0 && x < insize) ? r[x] : 0; }
        uint8_t e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < 16; ++k) e[p] |= t[p + k];
        o = make_uchar4(e[0] ? 1 : 0, e[1] ? 1 : 0, e[2] ? 1 : 0, e[3] ? 1 : 0);
    } else {
        uint32_t acc = 0;
        for (int k = -8; k <= 7; ++k) {
            const int yy = y + k;
            if (yy >= 0 && yy < insize) acc |= *reinterpret_cast<const uint32_t*>(img + (size_t)yy * insize + x0);
        }
        o = make_uchar4((acc & 0xffu) ? 1 : 0, (acc & 0xff00u) ? 1 : 0, (acc & 0xff0000u) ? 1 : 0, (acc & 0xff000000u) ? 1 : 0);
    }
    *reinterpret_cast<uchar4*>(out + row * insize + x0) = o;
}

}  // namespace

extern "C" int pmx_samples_prepare(pmx_ctx* c, const pmx_sample* samples, int n, int insize, int on_device)
{
    PMX_CHECK(c && samples, PMX_ERR_INVALID, "pmx_samples_prepare: null arg");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_samples_prepare: posenet contexts only (the samples are those of CocoPoseNet's data loader)");
    PMX_CHECK(n > 0, PMX_ERR_INVALID, "pmx_samples_prepare: n = %d", n);
    PMX_CHECK(insize > 0 && insize % 8 == 0, PMX_ERR_INVALID, "pmx_samples_prepare: insize %d must be a positive multiple of 8", insize);
    PMX_CHECK(n <= c->max_batch, PMX_ERR_CAPACITY, "pmx_samples_prepare: %d samples exceed max_batch %d", n, c->max_batch);
    PMX_CHECK((size_t)insize * insize <= (size_t)c->max_h * c->max_w, PMX_ERR_CAPACITY, "pmx_samples_prepare: insize %d exceeds the context capacity %d x %d",
              insize, c->max_h, c->max_w);
    const int LIM = 1 << 14;                                  // largest side of any image of a sample
    static const int RANGE[3] = {10, 40, 30};                 // distort_color's offsets (:167-169)
    // the layout of the staging block [descriptors | resize tables | images and masks (host sources only)] and of the intermediate images
    size_t tab_ints = 0, src_bytes = 0, a_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const pmx_sample& s = samples[i];
        PMX_CHECK(s.bgr, PMX_ERR_INVALID, "pmx_samples_prepare: sample %d has no image", i);
        PMX_CHECK(s.src_h >= 1 && s.src_w >= 1 && s.src_h <= LIM && s.src_w <= LIM, PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: source size %d x %d", i,
                  s.src_h, s.src_w);
        const bool rs = s.resized_w != 0 || s.resized_h != 0;
        PMX_CHECK(!rs || (s.resized_w >= 1 && s.resized_h >= 1 && s.resized_w <= LIM && s.resized_h <= LIM), PMX_ERR_INVALID,
                  "pmx_samples_prepare: sample %d: resized size %d x %d", i, s.resized_h, s.resized_w);
        if (!s.has_crop) {
            PMX_CHECK(!rs && !s.has_rotate && !s.has_distort && !s.flip, PMX_ERR_INVALID,
                      "pmx_samples_prepare: sample %d: a sample without the crop is a validation sample and has only the final resize", i);
            tab_ints += (size_t)8 * insize;
        } else {
            if (rs) { tab_ints += (size_t)4 * (s.resized_w + s.resized_h); a_bytes += pmx_align_up((size_t)s.resized_w * s.resized_h * 3, 16) + pmx_align_up((size_t)s.resized_w * s.resized_h, 16); }
            if (s.has_rotate) {
                PMX_CHECK(s.rot_w >= 1 && s.rot_h >= 1 && s.rot_w <= LIM && s.rot_h <= LIM, PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: rotated size %d x %d",
                          i, s.rot_h, s.rot_w);
                for (int k = 0; k < 6; ++k)
                    PMX_CHECK(isfinite(s.inv[k]) && fabs(s.inv[k]) <= 1e9, PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: matrix entry %d = %g", i, k, s.inv[k]);
                PMX_CHECK(s.inv[0] * s.inv[4] - s.inv[1] * s.inv[3] != 0, PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: singular matrix", i);
            }
            PMX_CHECK(abs(s.off_x) <= (1 << 20) && abs(s.off_y) <= (1 << 20), PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: crop offset", i);
            if (s.has_distort)
                for (int k = 0; k < 3; ++k)
                    PMX_CHECK(abs(s.delta[k]) <= RANGE[k], PMX_ERR_INVALID, "pmx_samples_prepare: sample %d: colour offset %d = %d outside +-%d", i, k, s.delta[k],
                              RANGE[k]);
        }
        if (!on_device) src_bytes += pmx_align_up((size_t)s.src_h * s.src_w * 3, 16) + (s.mask ? pmx_align_up((size_t)s.src_h * s.src_w, 16) : 0);
    }
    const size_t desc_off = 0, tab_off = pmx_align_up((size_t)n * sizeof(SampleDev), 16), src_off = pmx_align_up(tab_off + tab_ints * sizeof(int), 16);
    const size_t stage_bytes = src_off + src_bytes;
    const size_t npix = (size_t)c->max_batch * insize * insize;
    const size_t total = stage_bytes + a_bytes + npix * 6 + CONST_BYTES;
    PMX_CHECK(total <= PMX_SAMPLES_WORKSPACE_BYTES, PMX_ERR_CAPACITY, "pmx_samples_prepare: %zu bytes of workspace exceed the budget of %zu", total,
              (size_t)PMX_SAMPLES_WORKSPACE_BYTES);
    PMX_DEV(c);
    int rc;
    char *host, *dev;
    c->sp_n = 0;
    if ((rc = c->sp.begin(stage_bytes, c->stream, &host, &dev)) || (rc = c->sp_a.ensure(a_bytes, c->stream))) return rc;
    if ((rc = c->sp_out.ensure(npix * 3, c->stream)) || (rc = c->sp_mask_raw.ensure(npix, c->stream)) || (rc = c->sp_mask_tmp.ensure(npix, c->stream)) ||
        (rc = c->sp_mask.ensure(npix, c->stream)))
        return rc;
    if (!c->sp_const.capacity()) {                           // built and uploaded once per context
        std::vector<char> host(CONST_BYTES);
        build_consts(host.data());
        if ((rc = c->sp_const.alloc(CONST_BYTES))) return rc;
        if (hipMemcpy(c->sp_const, host.data(), CONST_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
            c->sp_const.reset();
            PMX_CHECK(false, PMX_ERR_HIP, "pmx_samples_prepare: upload of the weight tables failed");
        }
    }
    SampleDev* desc = (SampleDev*)(host + desc_off);
    size_t t = 0, so = src_off, ao = 0;
    int max_rs = 0, any_train = 0;
    for (int i = 0; i < n; ++i) {
        const pmx_sample& s = samples[i];
        SampleDev d;
        memset(&d, 0, sizeof d);
        d.sh = s.src_h; d.sw = s.src_w;
        const size_t px = (size_t)s.src_h * s.src_w;
        if (on_device) {
            d.src = s.bgr; d.msk = s.mask;
        } else {
            memcpy(host + so, s.bgr, px * 3);
            d.src = (const uint8_t*)dev + so; so += pmx_align_up(px * 3, 16);
            if (s.mask) { memcpy(host + so, s.mask, px); d.msk = (const uint8_t*)dev + so; so += pmx_align_up(px, 16); }
        }
        int* tabs = (int*)(host + tab_off) + t;
        const int* dtabs = (const int*)(dev + tab_off) + t;
        if (!s.has_crop) {
            d.rs_w = d.rs_h = insize;
            d.rs_img = c->sp_out + (size_t)i * insize * insize * 3;
            d.rs_msk = c->sp_mask_raw + (size_t)i * insize * insize;
        } else {
            d.train = 1; any_train = 1;
            d.a_img = d.src; d.a_msk = d.msk; d.ah = s.src_h; d.aw = s.src_w;
            if (s.resized_w) {
                d.rs_w = s.resized_w; d.rs_h = s.resized_h;
                const size_t rp = (size_t)d.rs_w * d.rs_h;
                d.rs_img = c->sp_a + ao; ao += pmx_align_up(rp * 3, 16);
                d.rs_msk = c->sp_a + ao; ao += pmx_align_up(rp, 16);
                d.a_img = d.rs_img; d.a_msk = s.mask ? d.rs_msk : nullptr; d.ah = d.rs_h; d.aw = d.rs_w;
            }
            d.rotate = s.has_rotate ? 1 : 0;
            d.rot_w = s.has_rotate ? s.rot_w : d.aw; d.rot_h = s.has_rotate ? s.rot_h : d.ah;
            for (int k = 0; k < 6; ++k) d.M[k] = s.has_rotate ? s.inv[k] : 0.0;
            d.ox = s.off_x; d.oy = s.off_y;
            d.distort = s.has_distort ? 1 : 0;
            for (int k = 0; k < 3; ++k) d.d[k] = s.has_distort ? s.delta[k] : 0;
            d.flip = s.flip ? 1 : 0;
        }
        if (d.rs_img) {
            pmx_make_resize_table(d.rs_w, s.src_w, tabs);
            pmx_make_resize_table(d.rs_h, s.src_h, tabs + 4 * d.rs_w);
            d.xtab = dtabs; d.ytab = dtabs + 4 * d.rs_w;
            t += (size_t)4 * (d.rs_w + d.rs_h);
            if (d.rs_w * d.rs_h > max_rs) max_rs = d.rs_w * d.rs_h;
        }
        desc[i] = d;
    }
    if ((rc = c->sp.commit(stage_bytes, c->stream))) return rc;
    const SampleDev* dd = (const SampleDev*)(dev + desc_off);
    const int32_t* wcub = (const int32_t*)c->sp_const.get();
    const int32_t* wlin = wcub + N_CUBIC;
    const int* sdiv = (const int*)(wlin + N_LINEAR);
    const int pix = insize * insize;
    if (max_rs) {
        if ((rc = pmx_prof_begin(c, "samples_resize|samples_resize", 0))) return rc;
        hipLaunchKernelGGL(samples_resize_kernel, dim3((max_rs + 255) / 256, n, 2), dim3(256), 0, c->stream, dd);
        PMX_HIP(hipGetLastError());
        if ((rc = pmx_prof_end(c))) return rc;
    }
    if (any_train) {
        if ((rc = pmx_prof_begin(c, "samples_window|samples_window", 0))) return rc;
        hipLaunchKernelGGL(samples_window_kernel, dim3((pix + 255) / 256, n), dim3(256), 0, c->stream, dd, wcub, wlin, sdiv, sdiv + 256,
                           (uint8_t*)c->sp_out, (uint8_t*)c->sp_mask_raw, insize);
        PMX_HIP(hipGetLastError());
        if ((rc = pmx_prof_end(c))) return rc;
    }
    const unsigned nb = (unsigned)(((size_t)n * pix / 4 + 255) / 256);
    if ((rc = pmx_prof_begin(c, "samples_dilate|samples_dilate", 0))) return rc;
    hipLaunchKernelGGL(samples_dilate_kernel<true>, dim3(nb), dim3(256), 0, c->stream, (const uint8_t*)c->sp_mask_raw, (uint8_t*)c->sp_mask_tmp, n, insize);
    hipLaunchKernelGGL(samples_dilate_kernel<false>, dim3(nb), dim3(256), 0, c->stream, (const uint8_t*)c->sp_mask_tmp, (uint8_t*)c->sp_mask, n, insize);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    c->sp_n = n; c->sp_insize = insize;
    return PMX_OK;
}

extern "C" int pmx_samples_device_ptrs(pmx_ctx* c, void** bgr_nhwc, void** mask)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "pmx_samples_device_ptrs: null ctx");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_samples_device_ptrs: posenet contexts only");
    PMX_CHECK(c->sp_n > 0, PMX_ERR_STATE, "pmx_samples_device_ptrs: no prepared samples (call pmx_samples_prepare first)");
    if (bgr_nhwc) *bgr_nhwc = c->sp_out.get();
    if (mask) *mask = c->sp_mask.get();
    return PMX_OK;
}

extern "C" int pmx_get_samples(pmx_ctx* c, uint8_t* bgr, uint8_t* mask, int n, int insize)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "pmx_get_samples: null ctx");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_get_samples: posenet contexts only");
    PMX_CHECK(c->sp_n > 0, PMX_ERR_STATE, "pmx_get_samples: no prepared samples (call pmx_samples_prepare first)");
    PMX_CHECK(n == c->sp_n && insize == c->sp_insize, PMX_ERR_INVALID, "pmx_get_samples: %d samples of %d asked, %d of %d prepared", n, insize, c->sp_n,
              c->sp_insize);
    PMX_DEV(c);
    const size_t px = (size_t)n * insize * insize;
    if (bgr) PMX_HIP(hipMemcpyAsync(bgr, c->sp_out, px * 3, hipMemcpyDeviceToHost, c->stream));
    if (mask) PMX_HIP(hipMemcpyAsync(mask, c->sp_mask, px, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_validate_samples(pmx_ctx* c, const double* poses, const int* n_people, double* out13)
{
    PMX_CHECK(c && n_people && out13, PMX_ERR_INVALID, "pmx_validate_samples: null arg");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_validate_samples: posenet contexts only");
    PMX_CHECK(c->sp_n > 0, PMX_ERR_STATE, "pmx_validate_samples: no prepared samples (call pmx_samples_prepare first)");
    const int n = c->sp_n, s = c->sp_insize;
    if (int rc = pmx_loss_set_poses_masked(c, poses, n_people, n, s, s, c->sp_mask, /*mask_on_device=*/true, 7.0, 8.0)) return rc;
    return pmx_validate_batch(c, c->sp_out, n, s, s, 1, out13);
}
