// Host-only check of the index functions of submap extraction in ekf_device.h (extract_landmark, extract_block, extract_element:
// the code k_ext_tiles, k_ext_vec and k_ext_dense run).  A dense symmetric P_LL of DISTINCT values is packed into a source layout
// of Ts tiles per side as k_import packs it (Bm through bm_offset, the landmarks' own blocks also into D).  For selections that are
// increasing, reversed, shuffled, the full map and a single landmark, the destination -- a layout of ANOTHER tile count Td -- is
// gathered as k_ext_tiles walks it (the tile's landmarks mapped once, then every work item of reframe_item: two blocks, two 32-byte
// pieces, each block through extract_block and the two half-used pieces fuse_block loads) and must equal the packing of P[sel, sel]
// in every stored place: below the diagonal of a diagonal tile, the own blocks and the zeros beyond the new map included.  The dense
// read-out's element function must give P[sel, sel] element by element, and D' = the diagonal blocks.
#include <algorithm>
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

// the block P(a, c) of the source as fuse_block reads it: {(0,0), (0,1), (1,0), (1,1)}
static int read_block(int Ts, int dns, const std::vector<double> &Bm, const std::vector<double> &D, int a, int c, double m[4]) {
    const FuseSource s = extract_block(Ts, a, c);
    m[0] = m[1] = m[2] = m[3] = 0.0;
    if (s.where == EX_ZERO) return 0;
    if (s.where == FW_D) {
        if (s.off >= (size_t)dns) return printf("D source out of range\n"), 1;
        m[0] = D[s.off], m[1] = m[2] = D[dns + s.off], m[3] = D[2 * (size_t)dns + s.off];
        return 0;
    }
    const int half = (int)(s.off & 1);
    const size_t p = s.off - half;
    if (p % 4 != 0 || p + 36 > Bm.size()) return printf("Bm pieces outside the buffer or not aligned\n"), 1;
    const double t[4] = {Bm[p + half], Bm[p + 2 + half], Bm[p + 32 + half], Bm[p + 34 + half]};
    const bool tr = s.where == FW_BM_T;
    m[0] = t[0], m[1] = tr ? t[2] : t[1], m[2] = tr ? t[1] : t[2], m[3] = t[3];
    return 0;
}

static int check(int N, int Ts, int Td, const std::vector<int> &ids, const char *name) {
    const int m = 2 * N, dns = 32 * Ts, dnd = 32 * Td;
    std::vector<double> L((size_t)m * m);
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) L[(size_t)i * m + j] = L[(size_t)j * m + i] = 1.0 + (double)((size_t)i * (i + 1) / 2 + j);  // distinct
    const int cnt = (int)ids.size(), mr = 2 * cnt;
    if (lm_tiles(cnt) > Td) return printf("%s: the destination is too small for the test\n", name), 1;
    std::vector<double> Bm, D, want_Bm, want_D;
    pack(Ts, dns, L, m, Bm, D);
    std::vector<double> Lr((size_t)mr * mr);
    for (int i = 0; i < mr; i++)
        for (int j = 0; j < mr; j++) Lr[(size_t)i * mr + j] = L[(size_t)(2 * ids[i >> 1] + (i & 1)) * m + 2 * ids[j >> 1] + (j & 1)];
    pack(Td, dnd, Lr, mr, want_Bm, want_D);
    const int *ip = ids.empty() ? nullptr : ids.data();
    std::vector<double> got(want_Bm.size(), -1.0);
    std::vector<int> writes(want_Bm.size(), 0);
    for (int I = 0; I < Td; I++)
        for (int J = I; J < Td; J++) {
            int lm[64];
            for (int k = 0; k < 64; k++) lm[k] = extract_landmark(ip, cnt, 32 * (k < 32 ? I : J) + (k & 31));
            const size_t tile = bm_tile_base(Td, I, J);
            for (int q = 0; q < 512; q++) {
                const ReframeItem it = reframe_item(q);
                double o[2][4];
                for (int k = 0; k < 2; k++) {
                    const int a = lm[it.row[k] >> 1], c = lm[32 + (it.col >> 1)];
                    if (a >= N || c >= N) return printf("%s: source landmark out of range\n", name), 1;
                    if (read_block(Ts, dns, Bm, D, a, c, o[k])) return 1;
                }
                // item_store: value v of piece s is element (row[v & 1] + s, col + (v >> 1))
                const double piece[2][4] = {{o[0][0], o[1][0], o[0][1], o[1][1]}, {o[0][2], o[1][2], o[0][3], o[1][3]}};
                for (int s = 0; s < 2; s++)
                    for (int v = 0; v < 4; v++) {
                        const size_t at = tile + it.off + 32 * s + v;
                        if (at != bm_offset(Td, 64 * I + it.row[v & 1] + s, 64 * J + it.col + (v >> 1))) return printf("%s: a piece value is not where item_store puts it\n", name), 1;
                        got[at] = piece[s][v], writes[at]++;
                    }
            }
        }
    for (size_t o = 0; o < got.size(); o++) {
        if (writes[o] != 1) return printf("%s: place %zu written %d times\n", name, o, writes[o]), 1;
        if (got[o] != want_Bm[o]) return printf("%s: N=%d Ts=%d Td=%d: Bm place %zu differs (%g vs %g)\n", name, N, Ts, Td, o, got[o], want_Bm[o]), 1;
    }
    // D as k_ext_vec fills it, zeros behind the new map
    for (int c = 0; c < 3; c++)
        for (int l = 0; l < dnd; l++) {
            const int a = extract_landmark(ip, cnt, l);
            const double v = a >= 0 ? D[(size_t)c * dns + a] : 0.0;
            if (v != want_D[(size_t)c * dnd + l]) return printf("%s: D element differs\n", name), 1;
        }
    // the dense read-out, element by element, and its symmetry
    for (int i = 0; i < mr; i++)
        for (int j = 0; j < mr; j++) {
            const RmSource s = extract_element(Ts, dns, ip, cnt, i, j), st = extract_element(Ts, dns, ip, cnt, j, i);
            if (s.where == RM_ZERO || s.where != st.where || s.off != st.off) return printf("%s: element (%d, %d) and its mirror have different homes\n", name, i, j), 1;
            if (s.off >= (s.where == RM_D ? D.size() : Bm.size())) return printf("%s: element source out of range\n", name), 1;
            const double v = s.where == RM_D ? D[s.off] : Bm[s.off];
            if (v != Lr[(size_t)i * mr + j]) return printf("%s: dense element (%d, %d) differs\n", name, i, j), 1;
        }
    if (extract_element(Ts, dns, ip, cnt, mr, 0).where != RM_ZERO) return printf("%s: a row beyond the selection has a source\n", name), 1;
    return 0;
}

int main() {
    struct Layout {
        int N, Ts, Td;
    };
    const Layout layouts[] = {{1, 1, 1}, {33, 2, 1}, {33, 2, 3}, {64, 2, 5}, {100, 4, 3}, {200, 10, 3}, {200, 7, 8}};
    int cases = 0;
    for (const Layout &ly : layouts) {
        const int N = ly.N, room = 32 * ly.Td;
        std::vector<int> all(N);
        for (int l = 0; l < N; l++) all[l] = l;
        std::vector<int> shuffled = all;
        for (int l = N - 1; l > 0; l--) std::swap(shuffled[l], shuffled[rnd() % (l + 1)]);
        const int part = std::min(room, std::max(1, (2 * N) / 3));
        std::vector<int> inc, rev, shuf(shuffled.begin(), shuffled.begin() + part);
        for (int l = 0; l < N && (int)inc.size() < part; l++)
            if (l % 3 != 1 || N < 3) inc.push_back(l);
        rev.assign(inc.rbegin(), inc.rend());
        // a shuffled list that holds the tile edges of the source when it has them
        for (int edge : {0, 31, 32, 63, 64, N - 1})
            if (edge < N && std::find(shuf.begin(), shuf.end(), edge) == shuf.end()) shuf[rnd() % shuf.size()] = edge;
        std::sort(shuf.begin(), shuf.end());
        shuf.erase(std::unique(shuf.begin(), shuf.end()), shuf.end());
        for (int l = (int)shuf.size() - 1; l > 0; l--) std::swap(shuf[l], shuf[rnd() % (l + 1)]);
        if (check(N, ly.Ts, ly.Td, inc, "increasing") || check(N, ly.Ts, ly.Td, rev, "reversed") || check(N, ly.Ts, ly.Td, shuf, "shuffled")) return 1;
        if (check(N, ly.Ts, ly.Td, {N / 2}, "single") || check(N, ly.Ts, ly.Td, {}, "empty")) return 1;
        cases += 5;
        if (N <= room) {
            if (check(N, ly.Ts, ly.Td, all, "full") || check(N, ly.Ts, ly.Td, shuffled, "full, shuffled")) return 1;
            cases += 2;
        }
    }
    printf("extract map ok (%d cases)\n", cases);
    return 0;
}
