// pp_tables.h -- the table set every post-process launch reads (PPTables), its ONE memory layout and its ONE host-side builder.
// Plain host C++ without a HIP call: a stand-alone program can include it (tests/test_pp_tables_host.py).
//
//   grid block of an (out_h, out_w) map   [xi0 | xi1 | yi0 | yi1] ints, padded to 8 bytes, then [xlo | xhi | ylo | yhi] doubles; the
//                                          x arrays out_w long, the y arrays out_h long                      (pp_grid_bytes)
//   taps block                             2 * PMX_GAUSS_MAX_RADIUS + 1 doubles: the taps in front, zeros behind (pp_taps_bytes)
//
// A builder writes a block to host memory (8-byte aligned) and points the members of a PPTables at the address the same bytes will have
// on the device; the caller uploads.  Who owns one set places the taps behind its grid, who serves many grids places them once.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>

#define PMX_GAUSS_MAX_RADIUS 16

struct PPTables {            // device pointers into a grid block and a taps block
    int* xi0; int* xi1; double* xlo; double* xhi;   // per output column
    int* yi0; int* yi1; double* ylo; double* yhi;   // per output row
    double* gauss;                                   // 2r+1 taps
    int radius;
    int border_zero;   // 0: scipy 'reflect' (CPU branch, golden); 1: zero padding (reference GPU branch, :112-113)
    int nms_ge;        // 0: strict '>' against the 4 neighbours (:98-101); 1: '>=' (GPU branch, :123-126)
};

// corner-aligned up-sampling grid of one axis: np.linspace(0, in-1, num=out) + the corner indices / weights of Chainer's ResizeImages
// (F.resize_images; see oracle).  pp_grid_build is the only caller
inline void pmx_make_upsample_grid(int in, int out, int* i0, int* i1, double* lo, double* hi)
{
    const double start = 0.0, stop = (double)(in - 1);
    const int div = out - 1;
    const double delta = stop - start;
    const double step = div > 0 ? delta / (double)div : 0.0;
    for (int k = 0; k < out; ++k) {
        double u;
        if (div > 0) {
            if (step == 0.0) u = ((double)k / (double)div) * delta + start;
            else u = (double)k * step + start;
            if (k == out - 1 && out > 1) u = stop;
        } else {
            u = start;     // num == 1 -> [start]
        }
        const int f = (int)floor(u);
        const double wl = (double)(f + 1) - u, wh = u - (double)f;
        i0[k] = f < 0 ? 0 : (f > in - 1 ? in - 1 : f);
        i1[k] = f + 1 > in - 1 ? in - 1 : (f + 1 < 0 ? 0 : f + 1);
        lo[k] = wl; hi[k] = wh;
    }
}

// bytes of the int arrays, rounded up to the doubles' alignment (2 * (out_w + out_h) ints: the rounding never adds a byte)
inline size_t pp_grid_int_bytes(int out_h, int out_w) { return (2 * ((size_t)out_w + (size_t)out_h) * sizeof(int) + 7) / 8 * 8; }
inline size_t pp_grid_bytes(int out_h, int out_w)
{
    return pp_grid_int_bytes(out_h, out_w) + 2 * ((size_t)out_w + (size_t)out_h) * sizeof(double);
}

// the eight arrays of the grid block at `base`
inline void pp_grid_point(void* base, int out_h, int out_w, PPTables& t)
{
    const size_t w = (size_t)out_w, h = (size_t)out_h;
    int* ip = static_cast<int*>(base);
    double* dp = reinterpret_cast<double*>(static_cast<char*>(base) + pp_grid_int_bytes(out_h, out_w));
    t.xi0 = ip; t.xi1 = ip + w; t.yi0 = ip + 2 * w; t.yi1 = ip + 2 * w + h;
    t.xlo = dp; t.xhi = dp + w; t.ylo = dp + 2 * w; t.yhi = dp + 2 * w + h;
}

// The grid of an (in_h, in_w) map up-sampled to (out_h, out_w) -> the pp_grid_bytes(out_h, out_w) bytes at `host`; the eight grid members of
// t -> the same arrays from `dev` on.  flip_x: column x of the mirrored map = column out_w - 1 - x of the resized one (same samples, same
// arithmetic: the x arrays reversed)
inline void pp_grid_build(int in_h, int in_w, int out_h, int out_w, int flip_x, void* host, void* dev, PPTables& t)
{
    PPTables h;
    pp_grid_point(host, out_h, out_w, h);
    pmx_make_upsample_grid(in_w, out_w, h.xi0, h.xi1, h.xlo, h.xhi);
    if (flip_x) {
        std::reverse(h.xi0, h.xi0 + out_w); std::reverse(h.xi1, h.xi1 + out_w);
        std::reverse(h.xlo, h.xlo + out_w); std::reverse(h.xhi, h.xhi + out_w);
    }
    pmx_make_upsample_grid(in_h, out_h, h.yi0, h.yi1, h.ylo, h.yhi);
    pp_grid_point(dev, out_h, out_w, t);
}

inline size_t pp_taps_bytes() { return (size_t)(2 * PMX_GAUSS_MAX_RADIUS + 1) * sizeof(double); }

// The n <= 2 * PMX_GAUSS_MAX_RADIUS + 1 taps of a symmetric filter (radius (n - 1) / 2) -> the pp_taps_bytes() bytes at `host`, zeros behind
// them; t.gauss -> `dev`, and the radius and the two flags of t
inline void pp_taps_build(const double* taps, int n, int border_zero, int nms_ge, void* host, void* dev, PPTables& t)
{
    memset(host, 0, pp_taps_bytes());
    memcpy(host, taps, (size_t)n * sizeof(double));
    t.gauss = static_cast<double*>(dev);
    t.radius = (n - 1) / 2; t.border_zero = border_zero; t.nms_ge = nms_ge;
}
