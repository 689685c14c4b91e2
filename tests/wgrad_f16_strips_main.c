/* wgrad_f16_strips_main.c -- stand-alone driver of the f16 weight-gradient kernel's strip and group rule (csrc/wgrad_strips.h:
 * pmx_wgrad_f16_*), with the cap of include/pose_mi355x.h.  usage: wgrad_f16_strips_main B H W cout cin ks forced.  One line:
 * "blocks strips rows groups" -- the blocks of four waves per strip, the strips and the rows per strip of B * H image rows (forced: option
 * "wgrad_strips", 0 = automatic), the 16-pixel groups of an image row -- then "fp32 strips rows": pmx_conv2d_backward's fp32 rule for
 * the same layer, which the f16 rule stands beside. */
#include <stdio.h>
#include <stdlib.h>

#include "pose_mi355x.h"
#include "wgrad_strips.h"

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const int B = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), cout = atoi(argv[4]), cin = atoi(argv[5]), ks = atoi(argv[6]),
              forced = atoi(argv[7]);
    const int cg = (cout + 31) / 32 * 32, cx = (cin + 31) / 32 * 32;
    int rows = 0;
    const int strips = pmx_wgrad_f16_strips(B, H, cg, cx, ks, forced, PMX_WGRAD_MAX_STRIPS, &rows);
    printf("%d %d %d %d\n", pmx_wgrad_f16_blocks(cg, cx, ks), strips, rows, pmx_wgrad_f16_groups(W));
    const int s32 = pmx_wgrad_strips_cap(B, H, cg, cx, ks, forced, PMX_WGRAD_MAX_STRIPS, 0, &rows);
    printf("fp32 %d %d\n", s32, rows);
    return 0;
}
