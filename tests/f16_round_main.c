/* f16_round_main.c -- stand-alone driver of csrc/f16_round.h, the host's f16(v) of the f16 mode (the weight packer's rounding).
 * Reads float32 values from stdin until it ends, writes f16_rn_sat of each as a uint16 word to stdout (tests/test_f16_host.py). */
#include <stdint.h>
#include <stdio.h>

#include "f16_round.h"

int main(void)
{
    static float in[4096];
    static uint16_t out[4096];
    size_t n;
    while ((n = fread(in, sizeof in[0], 4096, stdin)) > 0) {
        for (size_t i = 0; i < n; ++i) out[i] = f16_rn_sat(in[i]);
        if (fwrite(out, sizeof out[0], n, stdout) != n) return 3;
    }
    return ferror(stdin) ? 2 : 0;
}
