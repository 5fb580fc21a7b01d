// Host-only check of the kept scratch's layout (ekf_map_scratch.h: Carver and the nine carve functions) and of the growth rule
// (ekf_map_plan.h: plan_grown_cap), called directly.  Every block, B in {1, 3}, capacities 1, 64, 65 (an odd dn / 32), 256 and 257
// (the gate's partial count changes), table capacities 64 and 128, list capacities 256 and 512:
// (a) the size a carve without a base yields is the closed-form byte count the hand-written reserve functions computed before the
//     carver existed (copied from them: this pins ekf_device_bytes);
// (b) carved over a malloc of exactly that size, every array -- over the extent its [B][..] comment documents, written down here a
//     second time -- is aligned for its type, keeps a tag of its own when all are filled (no two overlap), and the last ends at bytes();
// (c) plan_grown_cap against a brute-force loop for have, need in 0 .. 1100 at floors 64 and 256.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_map_plan.h"
#include "../../2d-ekf-slam_amd/csrc/ekf_map_scratch.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            printf("line %d (%s): %s does not hold\n", __LINE__, g_case, #cond);    \
            failures++;                                                             \
        }                                                                           \
    } while (0)
static char g_case[128] = "";

struct Array {
    const char *name;
    void *p;
    size_t bytes, align;
};
template <typename T>
static Array arr(const char *name, T *p, size_t count) {
    return {name, (void *)p, count * sizeof(T), alignof(T)};
}

// One block: carve (sc, carver) lays it out, arrays (sc) lists what it holds; `want` is the parent's byte count.
template <typename S, typename Carve, typename Arrays>
static void check_block(const char *block, size_t want, Carve carve, Arrays arrays) {
    const size_t at = strlen(g_case);
    snprintf(g_case + at, sizeof g_case - at, " %s", block);
    S sized = {}, sc = {};
    Carver size{nullptr};
    carve(sized, size);
    CHECK(size.bytes() == want);
    if (size.bytes() != want) printf("  %zu bytes, the parent's expression gives %zu\n", size.bytes(), want);
    for (const Array &a : arrays(sized)) CHECK(a.p == nullptr);
    char *mem = (char *)malloc(size.bytes());  // (exactly: a sanitizer build sees the first byte behind it)
    Carver c{mem};
    carve(sc, c);
    CHECK(c.bytes() == size.bytes());
    const std::vector<Array> all = arrays(sc);
    size_t sum = 0, end = 0;
    for (size_t i = 0; i < all.size(); i++) {
        const Array &a = all[i];
        const size_t off = (size_t)((char *)a.p - mem);
        CHECK(a.p != nullptr && off % a.align == 0 && (size_t)(uintptr_t)a.p % a.align == 0);
        CHECK(off + a.bytes <= size.bytes());
        if (off + a.bytes > size.bytes()) {
            printf("  %s ends at %zu of %zu\n", a.name, off + a.bytes, size.bytes());
            free(mem);
            g_case[at] = 0;
            return;  // (nothing is written out of bounds)
        }
        memset(a.p, (int)(i + 1), a.bytes);
        sum += a.bytes;
        end = off + a.bytes > end ? off + a.bytes : end;
    }
    for (size_t i = 0; i < all.size(); i++) {
        size_t bad = 0;
        for (size_t q = 0; q < all[i].bytes; q++) bad += ((unsigned char *)all[i].p)[q] != (unsigned char)(i + 1);
        CHECK(bad == 0);
        if (bad) printf("  %s: %zu bytes carry another array's tag\n", all[i].name, bad);
    }
    CHECK(end == size.bytes());  // the last array ends where the block does ...
    CHECK(sum == size.bytes());  // ... and there is no padding: the block is the sum of its arrays
    free(mem);
    g_case[at] = 0;
}

int main() {
    const int caps[5] = {1, 64, 65, 256, 257};
    for (int Bi = 0; Bi < 2; Bi++)
        for (int Ncap : caps) {
            const size_t B = Bi ? 3 : 1;
            const int T = (2 * Ncap + 63) / 64;  // plan_geometry (ekf_geometry.h)
            const ScratchGeom g = {B, Ncap, (size_t)64 * T, (size_t)((3 + 64 * T) + 63) / 64 * 64, (size_t)32 * T, (size_t)T * (T + 1) / 2 * 4096};
            const size_t rows = g.rows, xs = g.xs, dn = g.dn;
            snprintf(g_case, sizeof g_case, "B %zu Ncap %d", B, Ncap);
            if (Ncap == 65 || Ncap == 257 || Ncap == 1) {
                CHECK(((dn >> 5) & 1) == 1);  // an odd dn / 32
            }
            {  // factor_reserve
                const size_t nS = B * g.bm_stride, nrhs = B * rows * 4, nacc = B * FAC_ACC, nxt = B * xs;
                check_block<FactorScratch>(
                    "factor", (nS + nrhs + nacc + nxt) * sizeof(double) + B * sizeof(ekf_joint), [&](FactorScratch &s, Carver &c) { carve_factor(s, c, g); },
                    [&](const FactorScratch &s) {
                        return std::vector<Array>{arr("S", s.S, B * g.bm_stride), arr("rhs", s.rhs, B * rows * 4), arr("acc", s.acc, B * FAC_ACC), arr("xt", s.xt, B * xs),
                                                  arr("out", s.out, B)};
                    });
            }
            {  // dup_reserve: the base
                const size_t nbox = B * (size_t)(dn >> 5) * 4;
                check_block<DupScratch>(
                    "dup", nbox * sizeof(double) + B * 3 * sizeof(int), [&](DupScratch &s, Carver &c) { carve_dup(s, c, g); },
                    [&](const DupScratch &s) { return std::vector<Array>{arr("box", s.box, B * (dn / 32) * 4), arr("cnt", s.cnt, B * 2), arr("split", s.split, B)}; });
            }
            {  // fuse_reserve
                const int pcap = Ncap / 2 + 1;
                const size_t nwr = B * 4 * FUSE_MAX_COLS, nU = B * FUSE_MAX_COLS * FUSE_MAX_COLS, nint = B * ((size_t)pcap * 2 + 4);
                check_block<FuseScratch>(
                    "fuse", (nwr + nU) * sizeof(double) + nint * sizeof(int),
                    [&](FuseScratch &s, Carver &c) {
                        carve_fuse(s, c, g);
                        CHECK(s.pcap == pcap);
                    },
                    [&](const FuseScratch &s) {
                        return std::vector<Array>{arr("wr", s.wr, B * 4 * FUSE_MAX_COLS), arr("U", s.U, B * FUSE_MAX_COLS * FUSE_MAX_COLS), arr("pairs", s.pairs, B * pcap * 2),
                                                  arr("cnt", s.cnt, B),                   arr("done", s.done, B * 2),                       arr("m_round", s.m_round, B)};
                    });
            }
            {  // assoc_reserve
                const size_t per = EKF_MAX_PENDING * (2 + EKF_ASSOC_MAX_BRANCH);
                CHECK(sizeof(AssocResult) + per * sizeof(int) == 2328);
                check_block<AssocScratch>(
                    "assoc", B * (sizeof(AssocResult) + per * sizeof(int)), [&](AssocScratch &s, Carver &c) { carve_assoc(s, c, g); },
                    [&](const AssocScratch &s) {
                        return std::vector<Array>{arr("out", s.out, B), arr("ncand", s.ncand, B * 32), arr("cand", s.cand, B * 32 * 16), arr("ids", s.ids, B * 32)};
                    });
            }
            for (int zcap : {64, 128}) {
                const size_t z = (size_t)zcap;
                {  // match_reserve
                    const size_t nz = B * zcap * 2, nR = B * zcap * 4, nd = B * zcap, ntab = B * EKF_MAX_PENDING * MATCH_TAB;
                    check_block<MatchScratch>(
                        zcap == 64 ? "match 64" : "match 128", (nz + nR + nd + ntab) * sizeof(double) + (B * zcap + B) * sizeof(int),
                        [&](MatchScratch &s, Carver &c) {
                            carve_match(s, c, g, zcap);
                            CHECK(s.zcap == zcap);
                        },
                        [&](const MatchScratch &s) {
                            return std::vector<Array>{arr("z", s.z, B * z * 2),   arr("Rm", s.Rm, B * z * 4), arr("d2", s.d2, B * z), arr("tab", s.tab, B * EKF_MAX_PENDING * MATCH_TAB),
                                                      arr("ids", s.ids, B * z), arr("cnt", s.cnt, B)};
                        });
                }
                {  // gate_reserve: the tables
                    const int npart = (Ncap + GATE_THREADS - 1) / GATE_THREADS;
                    CHECK(npart == (Ncap <= 256 ? 1 : 2));
                    const size_t nz = B * zcap * 2, nR = B * zcap * 4, np = B * npart * (size_t)zcap, nd = B * zcap;
                    check_block<GateScratch>(
                        zcap == 64 ? "gate 64" : "gate 128", (nz + nR + np) * sizeof(double) + nd * sizeof(ekf_decision) + (2 * np + nd + 2 * B) * sizeof(int),
                        [&](GateScratch &s, Carver &c) {
                            carve_gate(s, c, g, zcap);
                            CHECK(s.zcap == zcap && s.npart == npart && s.ccap == 0 && s.list == nullptr);
                        },
                        [&](const GateScratch &s) {
                            return std::vector<Array>{arr("z", s.z, B * z * 2),         arr("Rm", s.Rm, B * z * 4),       arr("pd", s.pd, B * npart * z),
                                                      arr("near", s.near, B * z),       arr("pl", s.pl, B * npart * z), arr("ps", s.ps, B * npart * z),
                                                      arr("skip", s.skip, B * z),       arr("nz", s.nz, B),               arr("cnt", s.cnt, B)};
                        });
                }
                {  // add_reserve
                    const size_t ntab = B * add_tab_stride(zcap), nops = B * zcap * 8;
                    check_block<AddScratch>(
                        zcap == 64 ? "add 64" : "add 128", (ntab + nops) * sizeof(double),
                        [&](AddScratch &s, Carver &c) {
                            carve_add(s, c, g, zcap);
                            CHECK(s.zcap == zcap);
                        },
                        [&](const AddScratch &s) { return std::vector<Array>{arr("tab", s.tab, B * add_tab_stride(zcap)), arr("ops", s.ops, B * z * 2 * 4)}; });
                }
            }
            for (int cap : {256, 512}) {  // dup_reserve, gate_reserve: the lists
                check_block<DupScratch>(
                    cap == 256 ? "dup list 256" : "dup list 512", B * (size_t)cap * sizeof(ekf_dup_pair),
                    [&](DupScratch &s, Carver &c) {
                        carve_dup_list(s, c, g, cap);
                        CHECK(s.cap == cap && s.box == nullptr);
                    },
                    [&](const DupScratch &s) { return std::vector<Array>{arr("list", s.list, B * cap)}; });
                check_block<GateScratch>(
                    cap == 256 ? "gate list 256" : "gate list 512", B * (size_t)cap * sizeof(ekf_candidate),
                    [&](GateScratch &s, Carver &c) {
                        carve_gate_list(s, c, g, cap);
                        CHECK(s.ccap == cap && s.zcap == 0 && s.z == nullptr);
                    },
                    [&](const GateScratch &s) { return std::vector<Array>{arr("list", s.list, B * cap)}; });
            }
        }
    // Carver::take aligns for the type it hands out (no block of today's needs it: a char before a double does)
    {
        snprintf(g_case, sizeof g_case, "carver");
        Carver c{nullptr};
        c.take<char>(3);
        CHECK(c.bytes() == 3);
        c.take<int>(1);
        CHECK(c.bytes() == 8);
        c.take<char>(1);
        c.take<double>(2);
        CHECK(c.bytes() == 32);
        alignas(8) char mem[32];
        Carver d{mem};
        d.take<char>(3);
        CHECK((char *)d.take<int>(1) == mem + 4);
        d.take<char>(1);
        CHECK((char *)d.take<double>(2) == mem + 16 && d.bytes() == 32);
    }
    // ---- (c) the growth rule ----
    snprintf(g_case, sizeof g_case, "plan_grown_cap");
    for (int floor : {64, 256})
        for (int have = 0; have <= 1100; have++)
            for (int need = 0; need <= 1100; need++) {
                int want = floor;  // at least the floor and what the handle has, doubled until the need fits
                if (have > want) want = have;
                while (want < need) want += want;
                const int got = plan_grown_cap(have, need, floor);
                if (got != want) {
                    printf("plan_grown_cap(%d, %d, %d) = %d, want %d\n", have, need, floor, got, want);
                    failures++;
                }
            }
    CHECK(plan_grown_cap(0, 64, 64) == 64 && plan_grown_cap(0, 65, 64) == 128 && plan_grown_cap(0, 256, 256) == 256 && plan_grown_cap(0, 257, 256) == 512);
    CHECK(plan_grown_cap(0, 1024, 64) == 1024 && plan_grown_cap(0, 1025, 256) == 2048 && plan_grown_cap(512, 3, 64) == 512 && plan_grown_cap(0, 0, 256) == 256);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("map scratch ok\n");
    return 0;
}
