/* f16_round.h -- the f16 mode's f16(v) (option "precision" = 2, include/pose_mi355x.h): fp32 -> f16 bits, round-to-nearest-even, saturating
 * at +-65504; NaN stays NaN.  The f16 weight pack is this function of the direct pack, float by float (pack_index.h::pmx_pk_f16_value,
 * evaluated on the device by pmx_packs.hip); conv_f16_kernel rounds the activations the same way.  Plain C, no dependency, and under hipcc
 * callable from both sides: tests/f16_round_main.c compiles it with the host compiler and compares it with numpy.float16 over every f16
 * value, its neighbours and every midpoint (tests/test_f16_host.py). */
#ifndef PMX_F16_ROUND_H
#define PMX_F16_ROUND_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PMX_HD __host__ __device__
#else
#define PMX_HD
#endif

static inline PMX_HD uint16_t f16_rn_sat(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, ax = u & 0x7fffffffu;
    if (ax > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (ax >= 0x477fe000u) return (uint16_t)(sign | 0x7bffu);          /* |x| >= 65504 (and what would round above it): the largest finite */
    if (ax < 0x38800000u) {                                             /* below 2^-14: subnormal f16 (or zero), in units of 2^-24 */
        if (ax < 0x33000000u) return (uint16_t)sign;                    /* below 2^-25: rounds to zero (2^-25 itself is the tie -> even = 0) */
        const uint32_t e = ax >> 23, m = (ax & 0x7fffffu) | 0x800000u;
        const uint32_t shift = 126 - e;                                 /* value = m * 2^(e - 150) = (m >> (126 - e)) * 2^-24 */
        const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
        return (uint16_t)(sign | (q + (rem > half || (rem == half && (q & 1)))));
    }
    const uint32_t r = ax + 0xfffu + ((ax >> 13) & 1u);                 /* round the 23-bit mantissa to 10 bits (a carry bumps the exponent) */
    return (uint16_t)(sign | (((r >> 13) - (112u << 10)) & 0x7fffu));
}

#endif
