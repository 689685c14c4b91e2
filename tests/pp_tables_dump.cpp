// Stand-alone host program of tests/test_pp_tables_host.py: runs the table builder of csrc/pp_tables.h over the cases on its command line
// and prints, one JSON line per case, the bytes it wrote and where it pointed the members of the PPTables.
//   grid in_h in_w out_h out_w flip   |   taps n border_zero nms_ge   (the taps are 1, 2, .. n)
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "pp_tables.h"

static void hex(const std::vector<double>& buf, size_t bytes)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(buf.data());
    for (size_t i = 0; i < bytes; ++i) printf("%02x", p[i]);
}

int main(int argc, char** argv)
{
    for (int a = 1; a < argc;) {
        const bool grid = argv[a][0] == 'g';
        const int need = grid ? 5 : 3;
        if (a + need >= argc) return 2;
        int v[5];
        for (int k = 0; k < need; ++k) v[k] = atoi(argv[a + 1 + k]);
        a += 1 + need;
        const size_t bytes = grid ? pp_grid_bytes(v[2], v[3]) : pp_taps_bytes();
        // `host` starts as 0xab bytes: what the builder leaves unwritten shows.  `dev` stands for the device copy: only its address is used
        std::vector<double> host(bytes / sizeof(double)), dev(bytes / sizeof(double));
        memset(host.data(), 0xab, bytes);
        PPTables t;
        memset(&t, 0xab, sizeof(t));
        const char* d = reinterpret_cast<const char*>(dev.data());
        if (grid) {
            pp_grid_build(v[0], v[1], v[2], v[3], v[4], host.data(), dev.data(), t);
            printf("{\"kind\": \"grid\", \"in_h\": %d, \"in_w\": %d, \"out_h\": %d, \"out_w\": %d, \"flip\": %d, \"bytes\": %zu, ", v[0], v[1], v[2], v[3], v[4], bytes);
            printf("\"xi0\": %td, \"xi1\": %td, \"yi0\": %td, \"yi1\": %td, \"xlo\": %td, \"xhi\": %td, \"ylo\": %td, \"yhi\": %td, ", (const char*)t.xi0 - d,
                   (const char*)t.xi1 - d, (const char*)t.yi0 - d, (const char*)t.yi1 - d, (const char*)t.xlo - d, (const char*)t.xhi - d,
                   (const char*)t.ylo - d, (const char*)t.yhi - d);
        } else {
            std::vector<double> taps(v[0]);
            for (int k = 0; k < v[0]; ++k) taps[k] = (double)(k + 1);
            pp_taps_build(taps.data(), v[0], v[1], v[2], host.data(), dev.data(), t);
            printf("{\"kind\": \"taps\", \"n\": %d, \"bytes\": %zu, \"gauss\": %td, \"radius\": %d, \"border_zero\": %d, \"nms_ge\": %d, ", v[0], bytes,
                   (const char*)t.gauss - d, t.radius, t.border_zero, t.nms_ge);
        }
        printf("\"raw\": \"");
        hex(host, bytes);
        printf("\"}\n");
    }
    return 0;
}
