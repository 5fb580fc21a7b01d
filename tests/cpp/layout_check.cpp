// Host-only check of the HBM index maps in ekf_device.h: bm_offset must be a bijection from the
// stored (i', j') pairs onto [0, tiles*4096) and agree with the MFMA C/D fragment order the dense
// pass assumes; pair_offset must be a bijection onto the slot array with one landmark per 64-byte line.
// The tile-level helpers the rewrite kernels share (tri_tile_ij, bm_tile_base, lm_tiles) must agree with bm_offset's numbering.
#include <cstdio>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

int main() {
    const int T = 3, n = 64 * T;
    size_t total = (size_t)T * (T + 1) / 2 * 4096;
    std::vector<int> hit(total, 0);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            if ((i >> 6) > (j >> 6)) continue;
            size_t o = bm_offset(T, i, j);
            if (o >= total) return printf("out of range at %d %d\n", i, j), 1;
            hit[o]++;
        }
    for (size_t o = 0; o < total; o++)
        if (hit[o] != 1) return printf("offset %zu hit %d times\n", o, hit[o]), 1;
    // fragment order: inside a tile, chain (rc, cc), piece h, lane l, element e  <->  row 16rc + (l>>4) + 4(2h+e), col 16cc + (l&15)
    for (int I = 0; I < T; I++)
        for (int J = I; J < T; J++) {
            size_t t = (size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I);
            for (int ch = 0; ch < 16; ch++)
                for (int h = 0; h < 2; h++)
                    for (int l = 0; l < 64; l++)
                        for (int e = 0; e < 2; e++) {
                            int row = 64 * I + 16 * (ch >> 2) + (l >> 4) + 4 * (2 * h + e);
                            int col = 64 * J + 16 * (ch & 3) + (l & 15);
                            size_t want = t * 4096 + (size_t)ch * 256 + h * 128 + l * 2 + e;
                            if (bm_offset(T, row, col) != want) return printf("fragment order mismatch\n"), 1;
                        }
        }
    const int pairs = 3, rows = 64 * T;
    std::vector<int> fh((size_t)pairs * rows * 4, 0);
    for (int i = 0; i < n; i++)
        for (int p = 0; p < pairs; p++)
            for (int k = 0; k < 4; k++) fh[pair_offset(rows, i, p) + k]++;
    for (size_t o = 0; o < fh.size(); o++)
        if (fh[o] != 1) return printf("pair_offset %zu hit %d times\n", o, fh[o]), 1;
    // one landmark's two rows of a slot pair are one 64-byte line; a 16-row block is 512 contiguous bytes
    for (int p = 0; p < pairs; p++)
        for (int i = 0; i < n; i += 2)
            if (pair_offset(rows, i + 1, p) - pair_offset(rows, i, p) != 4 || (pair_offset(rows, i, p) % 8) != 0) return printf("landmark line mismatch\n"), 1;
    for (int Tt = 1; Tt <= 9; Tt++) {
        int t = 0;
        for (int I = 0; I < Tt; I++)
            for (int J = I; J < Tt; J++, t++) {  // storage order: every (I, J), I <= J < Tt, exactly once
                int gi, gj;
                tri_tile_ij(t, Tt, &gi, &gj);
                if (gi != I || gj != J) return printf("tri_tile_ij(%d, %d) = (%d, %d), want (%d, %d)\n", t, Tt, gi, gj, I, J), 1;
                if (bm_tile_base(Tt, I, J) != bm_offset(Tt, 64 * I, 64 * J)) return printf("bm_tile_base(%d, %d, %d) is not bm_offset's tile\n", Tt, I, J), 1;
                if (bm_tile_base(Tt, I, J) != (size_t)t * 4096) return printf("bm_tile_base(%d, %d, %d) is not tile %d\n", Tt, I, J, t), 1;
            }
        if (t != Tt * (Tt + 1) / 2) return printf("triangle of side %d has %d tiles\n", Tt, t), 1;
        if (bm_tile_base(Tt, Tt - 1, Tt - 1) + 4096 != (size_t)Tt * (Tt + 1) / 2 * 4096) return printf("last tile of side %d\n", Tt), 1;
    }
    if (lm_tiles(0) != 0) return printf("lm_tiles(0) = %d\n", lm_tiles(0)), 1;
    for (int nl = 1; nl <= 300; nl++)  // the last landmark row is 2 nl - 1
        if (lm_tiles(nl) != ((2 * nl - 1) >> 6) + 1) return printf("lm_tiles(%d) = %d\n", nl, lm_tiles(nl)), 1;
    printf("layout ok\n");
    return 0;
}
