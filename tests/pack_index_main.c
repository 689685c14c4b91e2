/* pack_index_main.c -- stand-alone driver of csrc/pack_index.h, the index arithmetic the host and the device weight packers share.
 * usage: pack_index_main cout cin ks kind.  Writes int64 words to stdout: [nch, cout_pad, cin_pad, t_nch, t_cout_pad, t_cout, planes],
 * the reference channel of every packed input channel (cin_pad words), then per OIHW element (n, ci, tap) its place in the direct pack
 * and in the transposed pack of the data gradient, then (ks > 1) the place of every (plane, n < cout_pad, ci < cin_pad) in the Winograd pack. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pack_index.h"

static void put(int64_t v) { fwrite(&v, sizeof v, 1, stdout); }

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
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
    return 0;
}
