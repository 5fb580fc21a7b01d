// Host-only check of the index functions of landmark fusion in ekf_device.h (fuse_source, fuse_slot_offset: the code k_fuse_gather,
// k_fuse_factor and k_fuse_apply run).  For T = 1, 2, 3, 5 tiles per side and every (row landmark l, column landmark c):
//   - the home fuse_source names holds element (e, f) of the block P(l, c) where the kernel takes it: a landmark's own block in D, a
//     block above the diagonal at bm_offset(2l + e, 2c + f) = off + 32 e + 2 f, one below it transposed, at bm_offset(2c + f, 2l + e)
//     = off + 32 f + 2 e;
//   - the kernel's two 32-byte pieces (at off - (off & 1) and 32 doubles on) are 32-byte aligned, stay inside the block's tile, and
//     their values (off & 1) and 2 + (off & 1) are the block (item_block of reframe_item's pieces);
// and for every row and column of a round: fuse_slot_offset is element (q & 3) of the row's four doubles of slot pair q >> 2
// (pair_offset), the two columns of a pair adjacent and 16-byte aligned, below the zero pair.
#include <cstdio>
#include <cstdlib>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static int check_source(int T) {
    const int n = 32 * T;
    for (int l = 0; l < n; l++)
        for (int c = 0; c < n; c++) {
            const FuseSource s = fuse_source(T, l, c);
            if (l == c) {
                if (s.where != FW_D || s.off != (size_t)l) return printf("T=%d: own block of %d not in D\n", T, l), 1;
                continue;
            }
            if (s.where != (l < c ? FW_BM : FW_BM_T)) return printf("T=%d: block (%d, %d): wrong orientation\n", T, l, c), 1;
            const int lo = l < c ? l : c, hi = l < c ? c : l;
            const size_t tile = bm_tile_base(T, (2 * lo) >> 6, (2 * hi) >> 6);
            const int half = (int)(s.off & 1);
            const size_t piece = s.off - half;
            if (piece % 4 != 0 || piece < tile || piece + 32 + 4 > tile + 4096) return printf("T=%d: block (%d, %d): pieces leave the tile or are not aligned\n", T, l, c), 1;
            for (int e = 0; e < 2; e++)
                for (int f = 0; f < 2; f++) {
                    // element (e, f) of P(l, c) is the stored element (row, col) of the upper triangle
                    const size_t home = l < c ? bm_offset(T, 2 * l + e, 2 * c + f) : bm_offset(T, 2 * c + f, 2 * l + e);
                    const size_t at = l < c ? s.off + 32 * e + 2 * f : s.off + 32 * f + 2 * e;
                    if (at != home) return printf("T=%d: block (%d, %d): element %d %d is not where the kernel reads it\n", T, l, c, e, f), 1;
                    // ... and value 2 * (stored column) + half of piece (stored row)
                    const int sr = l < c ? e : f, sc = l < c ? f : e;
                    if (piece + 32 * sr + 2 * sc + half != home) return printf("T=%d: block (%d, %d): piece value %d %d\n", T, l, c, sr, sc), 1;
                }
        }
    return 0;
}

static int check_slots(int T, int maxp) {
    const int rows = 64 * T, maxpairs = (maxp + 1) / 2;
    for (int ip = 0; ip < rows; ip++)
        for (int q = 0; q < 2 * maxp; q++) {
            const size_t at = fuse_slot_offset(rows, ip, q);
            if (at != pair_offset(rows, ip, q >> 2) + (q & 3)) return printf("T=%d: row %d column %d: not in its slot pair\n", T, ip, q), 1;
            if ((q & 1) == 0 && (at % 2 != 0 || fuse_slot_offset(rows, ip, q + 1) != at + 1)) return printf("T=%d: row %d: the columns of pair %d are not adjacent\n", T, ip, q >> 1), 1;
            if (at >= pair_offset(rows, 0, maxpairs)) return printf("T=%d: row %d column %d reaches the zero pair\n", T, ip, q), 1;
        }
    return 0;
}

int main() {
    int cases = 0;
    for (int T : {1, 2, 3, 5}) {
        if (check_source(T)) return 1;
        for (int maxp : {1, 4, 8, 16, 32})
            if (check_slots(T, maxp)) return 1;
        cases++;
    }
    printf("fuse map ok (%d layouts)\n", cases);
    return 0;
}
