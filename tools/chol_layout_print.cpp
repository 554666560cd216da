// Prints the Cholesky chain's host-side geometry (quantool_amd/csrc/chol_layout.h) without the library or a GPU:
// per K the workspace regions of one problem on the f32 chain and with plane products (max_slabs as given), and the
// block rows of the default block sizes.  Built on the host alone, so it can run under the sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/chol_layout_print.cpp -o chol_layout_print
//   ./chol_layout_print [max_slabs] [K ...]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../quantool_amd/csrc/chol_layout.h"

static void print_layout(int K, bool g3, int max_slabs) {
    const CholLayout L(K, g3, max_slabs);
    printf("K=%-6d %-4s T %zu TI %zu XT %zu Rd %zu Dinv %zu split %zu (+%zu) Rpl %zu Ypl %zu slabs %zu | bytes %zu  x3 + tables at %zu\n",
           K, g3 ? "g3" : "f32", L.T, L.TI, L.XT, L.Rd, L.Dinv, L.split, L.split_bytes, L.Rpl, L.Ypl, L.slabs, L.bytes(), L.tables(3));
}

int main(int argc, char** argv) {
    const int max_slabs = argc > 1 ? atoi(argv[1]) : 256;
    std::vector<int> Ks;
    for (int i = 2; i < argc; ++i) Ks.push_back(atoi(argv[i]));
    if (Ks.empty()) Ks = {128, 256, 384, 640, 1024, 1536, 4096, 4224, 8192, 14336, 28672};
    for (int K : Ks) {
        print_layout(K, false, 0);
        print_layout(K, true, max_slabs);
        for (int nb : {256, 512}) {
            int rows = 0, covered = 0;
            BlockRow last(K, nb);
            for (BlockRow J(K, nb); J; ++J) {
                if (J.J0 != covered || J.J1 <= J.J0 || J.J1 > K || J.Jb != rows) return 1;
                covered = J.J1;
                ++rows;
                last = J;
            }
            if (covered != K || rows != BlockRow::count(K, nb)) return 1;
            printf("         nb=%d: %d block rows, last [%d, %d) Tm %d Tn0 %d Tn1 %d c_end %d\n", nb, rows, last.J0, last.J1,
                   last.Tm(), last.Tn0(), last.Tn1(), last.c_end());
        }
    }
    return 0;
}
