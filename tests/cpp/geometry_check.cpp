// Host-only check of plan_geometry (csrc/ekf_geometry.h) against the table tests/golden/chain_geometry.csv, which was dumped from
// the text of create_impl before the function existed.  Every field of every row must agree; after an error only the status is compared.
#include <cstdio>
#include <cstring>

#include "../../2d-ekf-slam_amd/csrc/ekf_geometry.h"

int main(int argc, char **argv) {
    if (argc < 2) return printf("usage: geometry_check chain_geometry.csv\n"), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return printf("cannot open %s\n", argv[1]), 2;
    static const char *names[23] = {"is_overlap", "chain_wgs", "solo", "solo_kernel", "solo_long", "solo_fuse", "chain_filters", "lpw", "hpw", "nrec", "vs_cap", "maxp",
                                    "eff_max_pending", "chain_lds", "chain_threads", "chain_one", "T", "xs", "dn", "rows", "bm_stride", "maxpairs", "f_stride"};
    char line[1024];
    int rows = 0, bad = 0;
    while (fgets(line, sizeof line, f)) {
        long long v[36];
        int n = 0;
        for (char *tok = strtok(line, ",\n"); tok && n < 36; tok = strtok(nullptr, ",\n")) {
            char *end;
            v[n] = strtoll(tok, &end, 10);
            if (end == tok || *end) break;  // (the comment line and the column names)
            n++;
        }
        if (n == 0) continue;
        if (n != 36) return printf("row %d: %d fields, want 36\n", rows + 1, n), 2;
        rows++;
        ekf_params p;
        memset(&p, 0, sizeof p);
        p.max_pending = (int)v[2], p.overlap = (int)v[3], p.log_capacity = 4096;
        Tunables tn;
        EnvInt *env[7] = {&tn.overlap, &tn.solo, &tn.chain_wgs, &tn.solo_long_window, &tn.solo_fuse, &tn.chain_one, &tn.chain_helpers};
        for (int i = 0; i < 7; i++)
            if (v[5 + i] != -99) env[i]->set = true, env[i]->v = (int)v[5 + i];
        const ChainGeometry g = plan_geometry((int)v[0], (int)v[1], p, (size_t)v[4], tn);
        if (g.error != (int)v[12]) {
            printf("row %d (batch %lld, capacity %lld): status %d, want %lld\n", rows, v[0], v[1], g.error, v[12]);
            bad++;
            continue;
        }
        if (g.error) continue;
        const long long got[23] = {g.overlap, g.chain_wgs, g.solo, g.solo_kernel, g.solo_long, g.solo_fuse, g.chain_filters, g.lpw, g.hpw, g.nrec, g.cache_slots, g.max_pending,
                                   g.max_pending, (long long)g.chain_lds, g.chain_threads, g.chain_one, g.T, g.xs, g.dn, g.rows, (long long)g.bm_stride, g.maxpairs, (long long)g.f_stride};
        for (int i = 0; i < 23; i++)
            if (got[i] != v[13 + i]) {
                printf("row %d (batch %lld, capacity %lld, window %lld, overlap %lld, LDS %lld): %s = %lld, want %lld\n", rows, v[0], v[1], v[2], v[3], v[4], names[i], got[i], v[13 + i]);
                bad++;
            }
    }
    fclose(f);
    if (bad || rows < 100) return printf("geometry check FAILED: %d mismatches in %d rows\n", bad, rows), 1;
    printf("geometry ok: %d rows\n", rows);
    return 0;
}
