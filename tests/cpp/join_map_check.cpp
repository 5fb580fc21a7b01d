// Host-only check of the map-joining index functions in ekf_device.h (join_tile_ij, join_tile_count, join_source: the code
// k_join_tiles runs) against a brute-force dense model.  The source's landmark block, every element a value of its own, is packed
// into a tile layout of the SOURCE's capacity as k_import packs it (Bm through bm_offset, own blocks into D).  Then, for a destination
// of another capacity:
//   - the tile list covers exactly the stored tiles that hold a new column, each once, and nothing else;
//   - every stored destination element is classified as the dense model says (old / robot-derived / source / beyond the map), and a
//     source element fetched through join_source is the dense model's element; a whole 2x2 block lies at off + 32 e + 2 f;
//   - the elements of the joined upper triangle that come from the source map to pairwise different source places, and the
//     walk by work items (reframe_item) reaches every element of a tile exactly once.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static double value_of(int i, int j) { return i <= j ? 1.0 + i * 4096.0 + j : 1.0 + j * 4096.0 + i; }  // symmetric, unique per pair

static int check(int Ng, int Ns, int cap_src) {
    const int Ts = (2 * cap_src + 63) / 64, dns = 32 * Ts, ms = 2 * Ns;
    const int cap_dst = Ng + Ns + 7, T = (2 * cap_dst + 63) / 64;
    if (Ns > cap_src) return 0;
    std::vector<double> Bm((size_t)Ts * (Ts + 1) / 2 * 4096, 0.0), D((size_t)3 * dns, 0.0);
    for (int i = 0; i < ms; i++)
        for (int j = 0; j < ms; j++) {
            if ((i >> 6) > (j >> 6)) continue;
            Bm[bm_offset(Ts, i, j)] = value_of(i, j);
            if ((i >> 1) == (j >> 1) && i <= j) D[(size_t)((i & 1) + (j & 1)) * dns + (i >> 1)] = value_of(i, j);
        }
    // ---- the tile list ----
    const int J0 = Ng >> 5, J1 = (2 * (Ng + Ns) + 63) >> 6, count = join_tile_count(Ng, Ns);
    std::set<std::pair<int, int>> listed;
    for (int t = 0; t < count + 5; t++) {
        int I, J;
        const bool in = join_tile_ij(t, J0, J1, &I, &J);
        if (in != (t < count)) return printf("Ng=%d Ns=%d: tile %d of %d: inside = %d\n", Ng, Ns, t, count, (int)in), 1;
        if (!in) continue;
        if (I < 0 || I > J || J < J0 || J >= J1 || J >= T) return printf("Ng=%d Ns=%d: tile %d = (%d, %d) out of range\n", Ng, Ns, t, I, J), 1;
        if (!listed.insert({I, J}).second) return printf("Ng=%d Ns=%d: tile (%d, %d) listed twice\n", Ng, Ns, I, J), 1;
    }
    // ---- every stored element of the destination layout ----
    std::map<std::pair<int, size_t>, std::pair<int, int>> used;  // source place -> the (min, max) pair that reads it
    const int m_old = 2 * Ng, m_all = 2 * (Ng + Ns);
    for (int I = 0; I < T; I++)
        for (int J = I; J < T; J++) {
            bool has_new = false;
            for (int i = 64 * I; i < 64 * I + 64; i++)
                for (int j = 64 * J; j < 64 * J + 64; j++) {
                    const JoinSource s = join_source(Ng, Ns, Ts, dns, i, j);
                    const bool beyond = i >= m_all || j >= m_all, old = i < m_old && j < m_old;
                    const int want = beyond ? JM_ZERO : old ? JM_OLD : (i < m_old || j < m_old) ? JM_ROBOT : (i >> 1) == (j >> 1) ? JM_D : JM_BM;
                    if (s.where != want) return printf("Ng=%d Ns=%d: element (%d, %d) classified %d, want %d\n", Ng, Ns, i, j, s.where, want), 1;
                    if (!beyond && !old) has_new = true;
                    if (want != JM_BM && want != JM_D) continue;
                    if (s.si != i - m_old || s.sj != j - m_old) return printf("source rows of (%d, %d) wrong\n", i, j), 1;
                    const std::vector<double> &home = want == JM_BM ? Bm : D;
                    if (s.off >= home.size()) return printf("Ng=%d Ns=%d: source of (%d, %d) outside the source's buffer\n", Ng, Ns, i, j), 1;
                    if (home[s.off] != value_of(s.si, s.sj)) return printf("Ng=%d Ns=%d cap %d: element (%d, %d) reads %g, want %g\n", Ng, Ns, cap_src, i, j, home[s.off], value_of(s.si, s.sj)), 1;
                    if (want == JM_BM && !(i & 1) && !(j & 1) && i < j) {  // the whole block from its first element, as the kernel reads it
                        for (int e = 0; e < 2; e++)
                            for (int f = 0; f < 2; f++)
                                if (Bm[s.off + 32 * e + 2 * f] != value_of(s.si + e, s.sj + f)) return printf("block of (%d, %d): element %d %d is not at +32 e + 2 f\n", i, j, e, f), 1;
                    }
                    if (i <= j) {
                        auto key = std::make_pair(want, s.off);
                        auto it = used.find(key);
                        if (it != used.end() && it->second != std::make_pair(i, j)) return printf("Ng=%d Ns=%d: two elements read one source place\n", Ng, Ns), 1;
                        used[key] = {i, j};
                    }
                }
            if (has_new != (listed.count({I, J}) == 1)) return printf("Ng=%d Ns=%d: tile (%d, %d): holds a new column = %d, listed = %d\n", Ng, Ns, I, J, (int)has_new, (int)listed.count({I, J})), 1;
        }
    // every element of the source's upper triangle (own blocks: xx, xy, yy) is read by exactly one joined element
    if ((long)used.size() != (long)ms * (ms + 1) / 2) return printf("Ng=%d Ns=%d: %zu source places read, want %ld\n", Ng, Ns, used.size(), (long)ms * (ms + 1) / 2), 1;
    return 0;
}

int main() {
    // the walk of a tile by work items: every tile-local offset once, whole 2x2 blocks
    std::vector<int> seen(4096, 0);
    for (int q = 0; q < 512; q++) {
        const ReframeItem it = reframe_item(q);
        for (int s = 0; s < 2; s++)
            for (int v = 0; v < 4; v++) {
                const int o = it.off + 32 * s + v;
                int il, jl;
                bm_tile_coords(o, &il, &jl);
                if (il != it.row[v & 1] + s || jl != it.col + (v >> 1)) return printf("work item %d: value %d of piece %d is not where the kernel thinks\n", q, v, s), 1;
                seen[o]++;
            }
    }
    for (int o = 0; o < 4096; o++)
        if (seen[o] != 1) return printf("tile offset %d visited %d times\n", o, seen[o]), 1;
    const int ngs[] = {0, 1, 31, 32, 33, 45, 100}, nss[] = {1, 31, 32, 33, 70}, caps[] = {96, 256};
    int cases = 0;
    for (int Ng : ngs)
        for (int Ns : nss)
            for (int cap : caps) {
                if (check(Ng, Ns, cap)) return 1;
                cases++;
            }
    if (join_tile_count(40, 0) != 0) return printf("an empty source has no tiles\n"), 1;
    printf("join map ok (%d cases)\n", cases);
    return 0;
}
