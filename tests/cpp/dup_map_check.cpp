// Host-only check of the pair enumeration of the duplicate search in ekf_device.h (dup_tile_count, dup_tile_ij, dup_pair: the code
// k_dup_tiles runs) by brute force.  For every map size N and every valid split:
//   - the tile list names stored tiles (I <= J < tiles of the map), each once, and ends where dup_tile_count says;
//   - walking every listed tile by work item (reframe_item) and block produces every considered pair (i < j < N; with a split:
//     i < split <= j) exactly once and nothing else;
//   - the four values the kernel takes for the pair (item_load / item_block: value k and 2 + k of the pieces at off and off + 32) are
//     P_ij[0][0], [0][1], [1][0], [1][1] at their homes in a layout of a LARGER capacity (bm_offset), above the diagonal.
// And the gate itself (dup_gate) against a long double restatement, the box gap (dup_box_gap, dup_dist2) as a lower bound of every
// pair's squared distance.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

static int check(int N, int split) {
    const int cap = N + 41, T = lm_tiles(cap), nT = lm_tiles(N);
    const int count = dup_tile_count(N, split);
    std::map<std::pair<int, int>, int> tiles, pairs;
    for (int t = -1; t < count + 5; t++) {
        int I = -1, J = -1;
        const bool in = dup_tile_ij(t, N, split, &I, &J);
        if (in != (t >= 0 && t < count)) return printf("N=%d split=%d: tile %d of %d: inside = %d\n", N, split, t, count, (int)in), 1;
        if (!in) continue;
        if (I < 0 || I > J || J >= nT) return printf("N=%d split=%d: tile %d = (%d, %d) is no stored tile of the map\n", N, split, t, I, J), 1;
        if (tiles[{I, J}]++) return printf("N=%d split=%d: tile (%d, %d) listed twice\n", N, split, I, J), 1;
        for (int q = 0; q < 512; q++) {
            const ReframeItem it = reframe_item(q);
            for (int k = 0; k < 2; k++) {
                int i, j;
                if (!dup_pair(N, split, I, J, it, k, &i, &j)) continue;
                pairs[{i, j}]++;
                // value v of piece s is element (row[v & 1] + s, col + (v >> 1)); block k = values k and 2 + k of both pieces
                for (int s = 0; s < 2; s++)
                    for (int f = 0; f < 2; f++) {
                        const size_t at = bm_tile_base(T, I, J) + it.off + 32 * s + 2 * f + k;
                        if (at != bm_offset(T, 2 * i + s, 2 * j + f)) return printf("N=%d: pair (%d, %d): element %d %d is not where the kernel reads it\n", N, i, j, s, f), 1;
                    }
            }
        }
    }
    long want = 0;
    for (int i = 0; i < N; i++)
        for (int j = i + 1; j < N; j++) {
            if (split > 0 && !(i < split && j >= split)) continue;
            want++;
            auto it = pairs.find({i, j});
            if (it == pairs.end() || it->second != 1) return printf("N=%d split=%d: pair (%d, %d) produced %d times\n", N, split, i, j, it == pairs.end() ? 0 : it->second), 1;
        }
    if ((long)pairs.size() != want) return printf("N=%d split=%d: %zu pairs produced, %ld considered\n", N, split, pairs.size(), want), 1;
    return 0;
}

static double rnd() { return rand() / (double)RAND_MAX; }

int main() {
    const int ns[] = {1, 2, 31, 32, 33, 64, 65, 100};
    int cases = 0;
    for (int N : ns) {
        const int splits[] = {0, 1, 31, 32, 33, N - 1, N};
        std::map<int, int> done;
        for (int sp : splits) {
            if (sp < 0 || sp > N || done[sp]++) continue;
            if (check(N, sp)) return 1;
            cases++;
        }
    }
    srand(7);
    double worst = 0.0;
    for (int t = 0; t < 20000; t++) {
        // own blocks and a cross block of their size; S stays well conditioned (a, c >= 0.4, |b| <= 0.2)
        const double di[3] = {1.0 + rnd(), 0.1 * (rnd() - 0.5), 1.0 + rnd()}, dj[3] = {1.0 + rnd(), 0.1 * (rnd() - 0.5), 1.0 + rnd()};
        const double pij[4] = {0.8 * rnd(), 0.1 * (rnd() - 0.5), 0.1 * (rnd() - 0.5), 0.8 * rnd()};
        const double dx = rnd() - 0.5, dy = rnd() - 0.5;
        double d2 = -1.0;
        const int deg = dup_gate(dx, dy, di, dj, pij, &d2);
        const long double a = (long double)di[0] + dj[0] - 2.0L * pij[0], b = (long double)di[1] + dj[1] - pij[1] - pij[2], c = (long double)di[2] + dj[2] - 2.0L * pij[3];
        const long double det = a * c - b * b;
        if (deg != !(a > 0 && det > 0)) return printf("gate: degenerate = %d, long double says %d\n", deg, (int)!(a > 0 && det > 0)), 1;
        if (deg) continue;
        const long double ref = (c * dx * dx - 2.0L * b * dx * dy + a * dy * dy) / det;
        const double err = (double)fabsl((d2 - ref) / ref);
        worst = err > worst ? err : worst;
    }
    if (worst > 1e-9) return printf("gate: worst relative error %.3e against long double\n", worst), 1;
    const double nan = std::nan("");
    double d2;
    const double one[3] = {1.0, 0.0, 1.0}, zero4[4] = {0.0, 0.0, 0.0, 0.0}, same[4] = {1.0, 0.0, 0.0, 1.0}, bad[4] = {nan, 0.0, 0.0, 0.0};
    if (dup_gate(1.0, 0.0, one, one, zero4, &d2) != 0 || d2 != 0.5) return printf("gate: independent unit blocks\n"), 1;
    if (dup_gate(0.0, 0.0, one, one, same, &d2) != 1) return printf("gate: S = 0 is degenerate\n"), 1;
    if (dup_gate(0.0, 0.0, one, one, bad, &d2) != 1) return printf("gate: NaN is degenerate\n"), 1;
    // the gap between two boxes never exceeds a pair's squared distance
    for (int t = 0; t < 20000; t++) {
        double pa[4][2], pb[4][2], ba[4] = {1e300, -1e300, 1e300, -1e300}, bb[4] = {1e300, -1e300, 1e300, -1e300};
        for (int k = 0; k < 4; k++) {
            pa[k][0] = 10.0 * rnd(), pa[k][1] = 10.0 * rnd(), pb[k][0] = 3.0 + 10.0 * rnd(), pb[k][1] = 10.0 * rnd() - 4.0;
            ba[0] = fmin(ba[0], pa[k][0]), ba[1] = fmax(ba[1], pa[k][0]), ba[2] = fmin(ba[2], pa[k][1]), ba[3] = fmax(ba[3], pa[k][1]);
            bb[0] = fmin(bb[0], pb[k][0]), bb[1] = fmax(bb[1], pb[k][0]), bb[2] = fmin(bb[2], pb[k][1]), bb[3] = fmax(bb[3], pb[k][1]);
        }
        const double gap = dup_dist2(dup_box_gap(ba[0], ba[1], bb[0], bb[1]), dup_box_gap(ba[2], ba[3], bb[2], bb[3]));
        for (int k = 0; k < 4; k++)
            for (int l = 0; l < 4; l++)
                if (gap > dup_dist2(pa[k][0] - pb[l][0], pa[k][1] - pb[l][1])) return printf("box gap %.17g exceeds a pair's squared distance\n", gap), 1;
    }
    printf("dup map ok (%d cases), gate worst relative error %.2e\n", cases, worst);
    return 0;
}
