/* pack_index_main.c -- stand-alone driver of csrc/pack_index.h, the definition of the weight packs the device packers evaluate.
 * usage: pack_index_main cout cin ks kind [weights [16]].  Writes int64 words to stdout: [nch, cout_pad, cin_pad, t_nch, t_cout_pad, t_cout, planes],
 * the reference channel of every packed input channel (cin_pad words), then per OIHW element (n, ci, tap) its place in the direct pack
 * and in the transposed pack of the data gradient, then (ks > 1) the place of every (plane, n < cout_pad, ci < cin_pad) in the Winograd pack.
 * With `weights`, a file of cout * cin * ks^2 + cout floats (w OIHW | b), the value functions follow as float32, every float of every pack
 * in index order: the direct pack, the padded bias, the transposed pack, (ks > 1) the Winograd packs of both, (a 64 x 3 x 3 x 3 layer)
 * conv1_1's fused-kernel pack, and the un-pack of the direct pack and bias; then, with `16`, as uint16 words the f16 pack and the bf16x3
 * pack of the direct pack. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pack_index.h"

static void put(int64_t v) { fwrite(&v, sizeof v, 1, stdout); }
static void put16(uint16_t v) { fwrite(&v, sizeof v, 1, stdout); }

/* every float of one pack through its value function */
static float* build(float (*value)(const PackJob*, unsigned), PackJob* j, size_t total)
{
    float* dst = (float*)malloc(total * sizeof(float));
    if (!dst) exit(4);
    j->dst = dst; j->total = (unsigned)total;
    for (unsigned idx = 0; idx < j->total; ++idx) dst[idx] = value(j, idx);
    fwrite(dst, sizeof(float), total, stdout);
    return dst;
}

static void wino(const float* direct, int ks, int nch, int cout_pad)
{
    PackJob j = {0};
    j.src = direct; j.ks = ks; j.p.nch = nch; j.p.cout_pad = cout_pad;
    free(build(pmx_pk_wino_value, &j, (size_t)pmx_pk_wino_planes(ks) * (nch * PMX_PK_CK / 32) * cout_pad * 32));
}

int main(int argc, char** argv)
{
    if (argc < 5 || argc > 7) return 2;
    const int cout = atoi(argv[1]), cin = atoi(argv[2]), ks = atoi(argv[3]), kind = atoi(argv[4]), T = ks * ks;
    const int cin_pad = pmx_pk_cin_pad(kind, cin), nch = cin_pad / PMX_PK_CK, cout_pad = pmx_pk_cout_pad(cout);
    const int t_cin_pad = pmx_pk_t_cin_pad(cout), t_nch = t_cin_pad / PMX_PK_CK, t_cout = pmx_pk_t_cout(kind, cin), t_cout_pad = pmx_pk_cout_pad(t_cout);
    const int planes = ks > 1 ? pmx_pk_wino_planes(ks) : 0;
    put(nch); put(cout_pad); put(cin_pad); put(t_nch); put(t_cout_pad); put(t_cout); put(planes);
    for (int k = 0; k < cin_pad; ++k) put(pmx_pk_ref_of_packed(kind, k, cin));
    for (int n = 0; n < cout; ++n)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < T; ++tap) {
                if (pmx_pk_oihw(n, ci, tap, cin, T) != ((size_t)n * cin + ci) * T + tap) return 3;
                put((int64_t)pmx_pk_direct(tap, pmx_pk_packed_of_ref(kind, ci), n, nch, cout_pad));
                put((int64_t)pmx_pk_direct(T - 1 - tap, n, pmx_pk_packed_of_ref(kind, ci), t_nch, t_cout_pad));
            }
    for (int p = 0; p < planes; ++p)
        for (int n = 0; n < cout_pad; ++n)
            for (int ci = 0; ci < cin_pad; ++ci) put((int64_t)pmx_pk_wino(p, n, ci, cin_pad / 32, cout_pad));
    if (argc == 5) return 0;

    const size_t nmaster = (size_t)cout * cin * T + cout;
    float* master = (float*)malloc(nmaster * sizeof(float));
    FILE* f = fopen(argv[5], "rb");
    if (!master || !f || fread(master, sizeof(float), nmaster, f) != nmaster) return 5;
    fclose(f);
    const PackGeo geo = {cout, cin, T, kind, nch, cout_pad};
    PackJob jd = {0}, jb = {0}, jt = {0};
    jd.src = master; jd.p = geo;
    float* direct = build(pmx_pk_direct_value, &jd, (size_t)T * nch * cout_pad * PMX_PK_CK);
    jb.src = master; jb.p = geo;
    float* bias = build(pmx_pk_bias_value, &jb, (size_t)cout_pad);
    jt.src = master; jt.p = geo; jt.p.nch = t_nch; jt.p.cout_pad = t_cout_pad; jt.t_cout = t_cout;
    float* transposed = build(pmx_pk_transposed_value, &jt, (size_t)T * t_nch * t_cout_pad * PMX_PK_CK);
    if (ks > 1 && cin_pad % 32 == 0) wino(direct, ks, nch, cout_pad);
    if (ks > 1 && t_cin_pad % 32 == 0) wino(transposed, ks, t_nch, t_cout_pad);
    if (cout == 64 && cin == 3 && ks == 3) {
        PackJob jc = {0};
        jc.src = direct; jc.p.cout_pad = cout_pad;
        free(build(pmx_pk_conv1_value, &jc, PMX_PK_CONV1_FLOATS));
    }
    for (size_t i = 0; i < nmaster; ++i) {
        const float v = pmx_pk_unpack_value(direct, bias, geo, (unsigned)i);
        fwrite(&v, sizeof v, 1, stdout);
    }
    if (argc == 7) {
        PackJob jh = {0};
        jh.src = direct; jh.p.cout_pad = cout_pad;
        const size_t nd = (size_t)T * nch * cout_pad * PMX_PK_CK;
        for (size_t i = 0; i < nd; ++i) put16(pmx_pk_f16_value(&jh, (unsigned)i));
        for (size_t i = 0; i < 3 * nd; ++i) put16(pmx_pk_bf16x3_value(&jh, (unsigned)i));
    }
    free(transposed); free(bias); free(direct); free(master);
    return 0;
}
