// Host-only check of the landmark-removal gather in ekf_device.h (bm_tile_coords, remove_row, remove_source: the code k_rm_gather
// runs).  Random symmetric matrices are packed into the tile layout as k_import packs them (Bm through bm_offset, the landmarks' own
// 2x2 blocks also into D); for random keep masks every destination tile is gathered element by element and must equal the packing of
// the dense matrix with the removed rows and columns deleted -- every stored element, zeros beyond the reduced map included -- and the
// reduced D must equal its diagonal blocks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

// k_import's packing of the landmark block L (m x m, m = 2N) into Bm (side T tiles) and D (stride dn)
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

static int check(int N, int T, int mode) {
    const int m = 2 * N, dn = 32 * T;
    std::vector<double> L((size_t)m * m);
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) {
            double v = (double)(long long)(rnd() >> 11) * 0x1.0p-53 - 0.5 + (i == j ? 4.0 : 0.0);
            L[(size_t)i * m + j] = L[(size_t)j * m + i] = v;
        }
    std::vector<int> map;  // the kept landmarks in order
    for (int l = 0; l < N; l++) {
        bool keep = mode == 0 ? (rnd() % 3 != 0) : mode == 1 ? true : mode == 2 ? false : mode == 3 ? (l != 0) : (l < N / 3 || l >= N / 3 + 17);
        if (keep) map.push_back(l);
    }
    const int n_new = (int)map.size(), mr = 2 * n_new;
    std::vector<double> Bm, D, want_Bm, want_D;
    pack(T, dn, L, m, Bm, D);
    std::vector<double> Lr((size_t)mr * mr);
    for (int i = 0; i < mr; i++)
        for (int j = 0; j < mr; j++) Lr[(size_t)i * mr + j] = L[(size_t)(2 * map[i >> 1] + (i & 1)) * m + 2 * map[j >> 1] + (j & 1)];
    pack(T, dn, Lr, mr, want_Bm, want_D);
    // the gather, tile by tile as k_rm_gather walks it: the tile's rows and columns mapped once, then every tile-local offset
    std::vector<double> got(Bm.size(), -1.0);
    const int *mp = map.empty() ? nullptr : map.data();
    for (int I = 0; I < T; I++)
        for (int J = I; J < T; J++) {
            int srow[64], scol[64];
            for (int k = 0; k < 64; k++) srow[k] = remove_row(mp, n_new, 64 * I + k), scol[k] = remove_row(mp, n_new, 64 * J + k);
            const size_t t = (size_t)I * T - (size_t)I * (I - 1) / 2 + (J - I);
            for (int o = 0; o < 4096; o++) {
                int il, jl;
                bm_tile_coords(o, &il, &jl);
                if (bm_offset(T, 64 * I + il, 64 * J + jl) != t * 4096 + o) return printf("bm_tile_coords is not the inverse of bm_offset\n"), 1;
                const int si = srow[il], sj = scol[jl];
                if (si >= m || sj >= m) return printf("source row out of range\n"), 1;
                const RmSource s = remove_source(T, dn, si, sj);
                double v = 0.0;
                if (s.where == RM_BM) {
                    if (s.off >= Bm.size() || s.off / 4096 < t) return printf("Bm source outside the buffer or in front of its destination tile\n"), 1;
                    v = Bm[s.off];
                } else if (s.where == RM_D) {
                    if (s.off >= D.size()) return printf("D source out of range\n"), 1;
                    v = D[s.off];
                }
                got[t * 4096 + o] = v;
            }
        }
    for (size_t o = 0; o < got.size(); o++)
        if (got[o] != want_Bm[o]) return printf("N=%d mode %d: Bm element %zu differs (%g vs %g)\n", N, mode, o, got[o], want_Bm[o]), 1;
    // D compacted as k_rm_vec does it: D'[c][l'] = D[c][map[l']], zeros behind
    for (int c = 0; c < 3; c++)
        for (int l = 0; l < dn; l++) {
            const double v = l < n_new ? D[(size_t)c * dn + map[l]] : 0.0;
            if (v != want_D[(size_t)c * dn + l]) return printf("N=%d: D element differs\n", N), 1;
        }
    // the zero region beyond the reduced map, stated directly
    for (int i = 0; i < 64 * T; i++)
        for (int j = 0; j < 64 * T; j++) {
            if ((i >> 6) > (j >> 6) || (i < mr && j < mr)) continue;
            if (got[bm_offset(T, i, j)] != 0.0) return printf("N=%d: nonzero beyond the reduced map at %d %d\n", N, i, j), 1;
        }
    return 0;
}

int main() {
    const int sizes[] = {1, 31, 32, 33, 64, 200, 300};
    int cases = 0;
    for (int N : sizes) {
        const int T = (2 * N + 63) / 64 + (N % 2);  // sometimes a capacity larger than the map
        for (int mode = 0; mode < 5; mode++)
            for (int rep = 0; rep < (mode == 0 ? 4 : 1); rep++) {
                if (check(N, T, mode)) return 1;
                cases++;
            }
    }
    printf("remove map ok (%d cases)\n", cases);
    return 0;
}
