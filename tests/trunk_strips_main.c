/* trunk_strips_main.c -- stand-alone driver of csrc/wgrad_strips.h, the strip rules of the weight-gradient kernels, with the constants of
 * include/pose_mi355x.h.  usage: trunk_strips_main B H forced.  One line per trunk layer conv1_1 .. conv4_2 for a batch of B images of
 * height H: "name strips rows waves" under the trunk chain's rules (forced: option "wgrad_strips", 0 = automatic), then one line
 * "head strips rows" with pmx_conv2d_backward's rule for a 128 -> 128 7x7 layer at H / 8. */
#include <stdio.h>
#include <stdlib.h>

#include "pose_mi355x.h"
#include "wgrad_strips.h"

int main(int argc, char** argv)
{
    static const struct { const char* name; int cin, cout, level; } L[10] = {
        {"conv1_1", 3, 64, 0}, {"conv1_2", 64, 64, 0}, {"conv2_1", 64, 128, 1}, {"conv2_2", 128, 128, 1}, {"conv3_1", 128, 256, 2},
        {"conv3_2", 256, 256, 2}, {"conv3_3", 256, 256, 2}, {"conv3_4", 256, 256, 2}, {"conv4_1", 256, 512, 3}, {"conv4_2", 512, 512, 3}};
    if (argc != 4) return 2;
    const int B = atoi(argv[1]), H = atoi(argv[2]), forced = atoi(argv[3]);
    for (int t = 0; t < 10; ++t) {
        int rows = 0, strips, units = 1;
        if (t == 0) strips = pmx_wgrad_conv1_strips(B, H, forced, PMX_WGRAD_CONV1_STRIPS, &rows);
        else {
            units = pmx_wgrad_units(L[t].cout, L[t].cin, 3);
            strips = pmx_wgrad_strips_cap(B, H >> L[t].level, L[t].cout, L[t].cin, 3, forced, PMX_WGRAD_TRUNK_MAX_STRIPS, 1, &rows);
        }
        printf("%s %d %d %d\n", L[t].name, strips, rows, strips * units);
    }
    int rows = 0;
    const int strips = pmx_wgrad_strips_cap(B, H / 8, 128, 128, 7, forced, PMX_WGRAD_MAX_STRIPS, 0, &rows);
    printf("head %d %d\n", strips, rows);
    return 0;
}
