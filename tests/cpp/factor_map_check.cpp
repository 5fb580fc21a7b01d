// Host-only check of the index functions of the tile-blocked Cholesky in ekf_device.h (chol_trail_count, chol_trail_ij,
// chol_operand_offset: the code k_chol_trail runs) against brute force:
//   - the trailing grid of step k lists exactly the stored tiles (I, J) with k < I <= J < nT, each once;
//   - the operand offset of k-step s, block blk, lane l is the home (bm_offset) of element (4 s + (l >> 4), 16 blk + (l & 15)) of a
//     tile, even k-steps are 16-byte aligned and the odd one lies right behind;
//   - a trailing update walked as the kernel walks it -- wave w = output row block, accumulator register r of lane l = element
//     (4 r + (l >> 4), l & 15) of chain (w, cc), operands A[m][kk] = -U_ki[4 s + kk][16 w + m], B[kk][n] = U_kj[4 s + kk][16 cc + n]
//     fetched through chol_operand_offset -- equals the dense A_ij - U_ki^T U_kj, with every element of the tile written once.
#include <cmath>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static int check_grid(int nT, int k) {
    std::set<std::pair<int, int>> want, got;
    for (int I = k + 1; I < nT; I++)
        for (int J = I; J < nT; J++) want.insert({I, J});
    const int count = chol_trail_count(nT, k);
    if (count != (int)want.size()) return printf("nT=%d k=%d: count %d, want %d\n", nT, k, count, (int)want.size()), 1;
    for (int t = 0; t < count; t++) {
        int I, J;
        chol_trail_ij(t, nT, k, &I, &J);
        if (!want.count({I, J})) return printf("nT=%d k=%d: tile %d = (%d, %d) is not a trailing tile\n", nT, k, t, I, J), 1;
        if (!got.insert({I, J}).second) return printf("nT=%d k=%d: tile (%d, %d) listed twice\n", nT, k, I, J), 1;
    }
    return 0;
}

static int check_operands() {
    for (int s = 0; s < 16; s++)
        for (int blk = 0; blk < 4; blk++)
            for (int lane = 0; lane < 64; lane++) {
                const int o = chol_operand_offset(s, blk, lane);
                const size_t home = bm_offset(1, 4 * s + (lane >> 4), 16 * blk + (lane & 15));
                if (o < 0 || o >= 4096 || (size_t)o != home) return printf("operand s=%d blk=%d lane=%d: offset %d, home %zu\n", s, blk, lane, o, home), 1;
                if (!(s & 1) && ((o & 1) || chol_operand_offset(s + 1, blk, lane) != o + 1)) return printf("operand s=%d blk=%d lane=%d: not a 16-byte pair\n", s, blk, lane), 1;
            }
    return 0;
}

static int check_update() {
    std::vector<double> ui(4096), uj(4096), c(4096), out(4096, 0.0);
    std::vector<int> written(4096, 0);
    auto val = [](int salt, int r, int col) { return std::sin(0.37 * salt + 0.11 * r + 0.013 * col * (salt + 1)); };
    for (int r = 0; r < 64; r++)
        for (int col = 0; col < 64; col++) {
            ui[bm_offset(1, r, col)] = val(1, r, col);
            uj[bm_offset(1, r, col)] = val(2, r, col);
            c[bm_offset(1, r, col)] = val(3, r, col);
        }
    for (int w = 0; w < 4; w++)
        for (int cc = 0; cc < 4; cc++)
            for (int lane = 0; lane < 64; lane++)
                for (int reg = 0; reg < 4; reg++) {
                    const int at = (w * 4 + cc) * 256 + (reg >> 1) * 128 + lane * 2 + (reg & 1);  // as the kernel loads and stores its accumulators
                    const int m = 4 * reg + (lane >> 4), n = lane & 15;
                    if ((size_t)at != bm_offset(1, 16 * w + m, 16 * cc + n)) return printf("accumulator w=%d cc=%d lane=%d reg=%d: not at home\n", w, cc, lane, reg), 1;
                    double acc = c[at];
                    for (int s = 0; s < 16; s++)
                        for (int kk = 0; kk < 4; kk++)  // the MFMA: lane kk * 16 + m of A, lane kk * 16 + n of B
                            acc += -ui[chol_operand_offset(s, w, kk * 16 + m)] * uj[chol_operand_offset(s, cc, kk * 16 + n)];
                    out[at] = acc;
                    written[at]++;
                }
    for (int o = 0; o < 4096; o++)
        if (written[o] != 1) return printf("update: offset %d written %d times\n", o, written[o]), 1;
    for (int r = 0; r < 64; r++)
        for (int col = 0; col < 64; col++) {
            double want = val(3, r, col);
            for (int kk = 0; kk < 64; kk++) want += -val(1, kk, r) * val(2, kk, col);
            if (std::fabs(out[bm_offset(1, r, col)] - want) > 1e-12) return printf("update: element (%d, %d) = %.17g, want %.17g\n", r, col, out[bm_offset(1, r, col)], want), 1;
        }
    return 0;
}

int main() {
    int grids = 0;
    for (int nT = 1; nT <= 14; nT++)
        for (int k = 0; k < nT; k++, grids++)
            if (check_grid(nT, k)) return 1;
    if (chol_trail_count(128, 0) != 127 * 128 / 2 || chol_trail_count(1, 0) != 0 || chol_trail_count(3, 2) != 0) return printf("trail count\n"), 1;
    if (check_operands()) return 1;
    if (check_update()) return 1;
    printf("factor map ok (%d grids)\n", grids);
    return 0;
}
