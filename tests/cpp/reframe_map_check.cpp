// Host-only check of the frame-change tile mapping in ekf_device.h (reframe_item, bm_chain_offset: the code k_reframe_tiles runs).
// For an off-diagonal and a diagonal tile: the 512 work items visit every element of the tile exactly once, each item's eight
// values are exactly the four elements of each of two 2x2 landmark blocks (even first row, even first column), and the offsets
// agree with bm_offset / bm_tile_coords.  Then the kernel's data movement is replayed on the host with an exactly representable
// rotation (Q = Rot(-90 deg): a permutation with signs) on a packed random symmetric matrix: every live chain must equal k_import's
// packing of the rotated matrix -- own blocks and below-diagonal places of the diagonal chains included -- and dead chains stay.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

static int check_items(int T, int I, int J) {
    const size_t t = (size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I);
    std::vector<int> seen(4096, 0), block_hits(32 * 32, 0);
    for (int q = 0; q < 512; q++) {
        const ReframeItem it = reframe_item(q);
        if (it.off < 0 || it.off + 32 + 3 >= 4096) return printf("item %d: offset outside the tile\n", q), 1;
        if ((it.row[0] & 1) || (it.col & 1) || it.row[1] != it.row[0] + 4) return printf("item %d: blocks do not start on even rows / columns\n", q), 1;
        if (it.chain != it.off >> 8 || it.chain != (it.off + 35) >> 8) return printf("item %d: leaves its chain\n", q), 1;
        for (int k = 0; k < 2; k++) block_hits[(it.row[k] >> 1) * 32 + (it.col >> 1)]++;
        for (int s = 0; s < 2; s++)
            for (int v = 0; v < 4; v++) {
                const int o = it.off + 32 * s + v, row = it.row[v & 1] + s, col = it.col + (v >> 1);
                int il, jl;
                bm_tile_coords(o, &il, &jl);
                if (il != row || jl != col) return printf("item %d piece %d value %d: (%d, %d) but bm_tile_coords says (%d, %d)\n", q, s, v, row, col, il, jl), 1;
                if (bm_offset(T, 64 * I + row, 64 * J + col) != t * 4096 + o) return printf("item %d: disagrees with bm_offset\n", q), 1;
                if (it.chain * 256 + bm_chain_offset(row & 15, col & 15) != o) return printf("item %d: disagrees with bm_chain_offset\n", q), 1;
                seen[o]++;
            }
    }
    for (int o = 0; o < 4096; o++)
        if (seen[o] != 1) return printf("tile offset %d visited %d times\n", o, seen[o]), 1;
    for (int k = 0; k < 32 * 32; k++)
        if (block_hits[k] != 1) return printf("block %d owned by %d items\n", k, block_hits[k]), 1;
    // a wave (64 consecutive items) covers two whole chains; its first and its second loads are each whole 256-byte runs
    for (int w = 0; w < 8; w++)
        for (int s = 0; s < 2; s++) {
            std::vector<int> hit(512, 0);
            for (int lane = 0; lane < 64; lane++)
                for (int v = 0; v < 4; v++) hit[reframe_item(64 * w + lane).off + 32 * s + v - 512 * w]++;
            for (int run = 0; run < 16; run++) {
                int cnt = 0;
                for (int k = 0; k < 32; k++) cnt += hit[32 * run + k];
                if (cnt != ((run & 1) == s ? 32 : 0)) return printf("wave %d load %d: not whole 256-byte runs\n", w, s), 1;
            }
        }
    return 0;
}

// k_import's packing of the landmark block L (m x m) into Bm (side T tiles) and D (stride dn)
static void pack(int T, int dn, const std::vector<double> &L, int m, std::vector<double> &Bm, std::vector<double> &D) {
    Bm.assign((size_t)T * (T + 1) / 2 * 4096, 0.0);
    D.assign((size_t)3 * dn, 0.0);
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            if ((i >> 6) > (j >> 6)) continue;
            Bm[bm_offset(T, i, j)] = L[(size_t)i * m + j];
            if ((i >> 1) == (j >> 1) && i <= j) D[(size_t)((i & 1) + (j & 1)) * dn + (i >> 1)] = L[(size_t)i * m + j];
        }
}

// Q B Q^T for Q = [[0, 1], [-1, 0]] (cos = 0, sin = 1), exact
static void rot90(const double b[4], double o[4]) { o[0] = b[3], o[1] = -b[2], o[2] = -b[1], o[3] = b[0]; }

static int check_replay(int N, int T) {
    const int m = 2 * N, dn = 32 * T, nT = (m + 63) / 64;
    std::vector<double> L((size_t)m * m), Lr((size_t)m * m);
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) L[(size_t)i * m + j] = L[(size_t)j * m + i] = (double)(long long)(rnd() >> 11) * 0x1.0p-53 - 0.5 + (i == j ? 4.0 : 0.0);
    for (int l = 0; l < N; l++)
        for (int k = 0; k < N; k++) {
            const double b[4] = {L[(size_t)(2 * l) * m + 2 * k], L[(size_t)(2 * l) * m + 2 * k + 1], L[(size_t)(2 * l + 1) * m + 2 * k], L[(size_t)(2 * l + 1) * m + 2 * k + 1]};
            double o[4];
            rot90(b, o);
            Lr[(size_t)(2 * l) * m + 2 * k] = o[0], Lr[(size_t)(2 * l) * m + 2 * k + 1] = o[1];
            Lr[(size_t)(2 * l + 1) * m + 2 * k] = o[2], Lr[(size_t)(2 * l + 1) * m + 2 * k + 1] = o[3];
        }
    std::vector<double> Bm, D, want, Dnew;
    pack(T, dn, L, m, Bm, D);
    pack(T, dn, Lr, m, want, Dnew);
    // stale places as in normal operation: own blocks and below-diagonal places of the diagonal tiles hold garbage
    for (int I = 0; I < nT; I++)
        for (int i = 0; i < 64; i++)
            for (int j = 0; j < 64; j++)
                if ((i >> 1) >= (j >> 1)) Bm[bm_offset(T, 64 * I + i, 64 * I + j)] = 1e30;
    const std::vector<double> before = Bm;
    for (int I = 0; I < nT; I++)
        for (int J = I; J < nT; J++) {
            double *tp = Bm.data() + ((size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I)) * 4096;
            for (int q = 0; q < 512; q++) {  // the work items, as k_reframe_tiles walks them
                const ReframeItem it = reframe_item(q);
                if (I == J && (it.chain >> 2) >= (it.chain & 3)) continue;
                const double *v0 = tp + it.off, *v1 = tp + it.off + 32;
                double o[2][4];
                for (int k = 0; k < 2; k++) {
                    const double b[4] = {v0[k], v0[2 + k], v1[k], v1[2 + k]};
                    rot90(b, o[k]);
                }
                const double s0[4] = {o[0][0], o[1][0], o[0][1], o[1][1]}, s1[4] = {o[0][2], o[1][2], o[0][3], o[1][3]};
                for (int v = 0; v < 4; v++) tp[it.off + v] = s0[v], tp[it.off + 32 + v] = s1[v];
            }
            if (I != J) continue;
            for (int tid = 0; tid < 256; tid++) {  // the diagonal chains: one lane per 2x2 block
                const int w = tid >> 6, a = (tid >> 3) & 7, c = tid & 7;
                if (a > c) continue;
                double *ch = tp + w * 5 * 256;
                if (a == c) {
                    const int l = 32 * I + 8 * w + a;
                    ch[bm_chain_offset(2 * a, 2 * a)] = Dnew[l], ch[bm_chain_offset(2 * a, 2 * a + 1)] = Dnew[dn + l];
                    ch[bm_chain_offset(2 * a + 1, 2 * a)] = Dnew[dn + l], ch[bm_chain_offset(2 * a + 1, 2 * a + 1)] = Dnew[2 * (size_t)dn + l];
                    continue;
                }
                double b[4], o[4];
                for (int d = 0; d < 2; d++)
                    for (int e = 0; e < 2; e++) b[2 * d + e] = ch[bm_chain_offset(2 * a + d, 2 * c + e)];
                rot90(b, o);
                for (int d = 0; d < 2; d++)
                    for (int e = 0; e < 2; e++) ch[bm_chain_offset(2 * a + d, 2 * c + e)] = o[2 * d + e], ch[bm_chain_offset(2 * c + e, 2 * a + d)] = o[2 * d + e];
            }
        }
    for (int I = 0; I < T; I++)
        for (int J = I; J < T; J++)
            for (int o = 0; o < 4096; o++) {
                const size_t at = ((size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I)) * 4096 + o;
                const int chain = o >> 8;
                const bool dead = J >= nT || (I == J && (chain >> 2) > (chain & 3));
                if (dead ? Bm[at] != before[at] : Bm[at] != want[at])
                    return printf("N=%d: tile (%d, %d) offset %d: %g, expected %g\n", N, I, J, o, Bm[at], dead ? before[at] : want[at]), 1;
            }
    return 0;
}

int main() {
    if (check_items(3, 0, 2) || check_items(3, 1, 1)) return 1;
    const int sizes[] = {1, 31, 32, 33, 64, 100};
    int cases = 0;
    for (int N : sizes) {
        if (check_replay(N, (2 * N + 63) / 64 + (N % 2))) return 1;
        cases++;
    }
    printf("reframe map ok (%d replays)\n", cases);
    return 0;
}
