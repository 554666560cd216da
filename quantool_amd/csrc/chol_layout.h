// Host-side geometry of the Cholesky chain (cholesky.hip): the block rows of a K x K matrix and one problem's share of
// the workspace.  Plain C++ with nothing of HIP in it, so that a stand-alone program can include it and print or
// sanitise it on the host (tools/chol_layout_print.cpp).  Internal linkage: one translation unit of the library uses it.
#pragma once
#include <stddef.h>

namespace {

constexpr int NB = 128;
constexpr int NBO_MAX = 1024; // workspace is sized for the widest outer block
constexpr int RD_STRIDE = NB * NB + 4 * 32 * 32;  // dense R block + four 32x32 sub-block inverses
constexpr int CHOL_TILE = 256, CHOL_CHUNK_ROWS = 64;   // gemm3_tn.h: output tile edge, granularity of an item's k range

constexpr size_t chol_align(size_t x) { return (x + 255) / 256 * 256; }

// Block row Jb of a K x K matrix cut into nb-row blocks: rows [J0, J1), the last one ragged.  Both phases walk these
// (outer blocks of the factorisation, block rows of the inverse), and so do the item tables of the row's two long
// products, whose shape in gemm3 tiles it states: Tm tile rows; Tn0 tile columns from J0 on (A[J, J0:], the factor's
// product), Tn1 left of J0 (T_J, the inverse's); k = J0 rows = c_end chunks.
//     for (BlockRow J(K, NBO); J; ++J) ...
struct BlockRow {
    int K, nb, J0, J1, Jb = 0;
    BlockRow(int K_, int nb_) : K(K_), nb(nb_) { at(0); }
    explicit operator bool() const { return J0 < K; }
    BlockRow& operator++() { at(J0 + nb); ++Jb; return *this; }
    static int count(int K, int nb) { return (K + nb - 1) / nb; }
    int rows() const { return J1 - J0; }
    int Tm() const { return (J1 - J0 + CHOL_TILE - 1) / CHOL_TILE; }
    int Tn0() const { return (K - J0 + CHOL_TILE - 1) / CHOL_TILE; }
    int Tn1() const { return (J0 + CHOL_TILE - 1) / CHOL_TILE; }
    int c_end() const { return J0 / CHOL_CHUNK_ROWS; }

  private:
    void at(int j0) { J0 = j0; J1 = (K - J0 < nb) ? K : J0 + nb; }
};

// ONE problem's share of the workspace, without the bf16x3 item tables (shared by a batch): byte offsets from the
// problem's 256-aligned base, each a multiple of 256 like every region's size.  g3 / max_slabs: CholG3Plan::any / max_slabs
// of the plan that sizes the workspace.
struct CholLayout {
    // T panel [128, K] + T_I panel [NBO_MAX, K] + X_II [NBO_MAX, NBO_MAX] + Rd [nb][RD_STRIDE], Dinv [nb][128*128] + split-K
    // slabs (a split product writes splits * M * N floats with splits <= 2048 workgroups / tiles: <= 2048 * 128 * 128)
    size_t T, TI, XT, Rd, Dinv, split, split_bytes;
    // bf16x3 products: plane copies of R and Y (three planes of K x K each), slabs
    size_t Rpl = 0, Ypl = 0, slabs = 0;

    CholLayout(int K, bool g3, int max_slabs) {
        const size_t nblk = (K + NB - 1) / NB;
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t o = chol_align(at); at = o + n; return o; };
        T = take((size_t)NB * K * 4);
        TI = take((size_t)NBO_MAX * K * 4);
        XT = take((size_t)NBO_MAX * NBO_MAX * 4);
        Rd = take(nblk * RD_STRIDE * 4);
        Dinv = take(nblk * NB * NB * 4);
        split_bytes = (size_t)2048 * NB * NB * 4 + (size_t)NBO_MAX * K * 4;
        split = take(split_bytes);
        size_t spare = 256;   // per part: room the size has always had and the carve does not use (no region needs padding)
        if (g3) {
            const size_t plane_bytes = chol_align((size_t)3 * K * K * 2);
            Rpl = take(plane_bytes);
            Ypl = take(plane_bytes);
            slabs = take((size_t)max_slabs * CHOL_TILE * CHOL_TILE * 4);
            spare += 256;
        }
        total = chol_align(at + spare);
    }
    size_t bytes() const { return total; }
    // A batch: nprob shares, then ONE copy of the item tables, + 512 for aligning the caller's base.
    size_t tables(int nprob) const { return (size_t)nprob * total; }
    size_t batch_bytes(int nprob, size_t table_bytes) const { return tables(nprob) + table_bytes + 512; }

  private:
    size_t total;
};

}  // namespace
