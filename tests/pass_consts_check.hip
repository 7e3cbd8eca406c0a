// Stand-alone check of the time loop's constants layout (ssmq_host.h: pass_consts_doubles, fill_pass_consts,
// wire_pass_consts), built with -fsanitize=address,undefined and run on the CPU by tests/test_pass_consts_layout.py.
// It calls no HIP API.  Exit status 0 and a last line "ok <cases>" mean every check held.
#include <cstdio>
#include <vector>
#include "ssmq_host.h"

using namespace ssmq;

static int g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            ++g_failed;                                                               \
            printf("FAILED line %d: %s  (%s)\n", __LINE__, #cond, what);              \
        }                                                                             \
    } while (0)

int main() {
    // a pair with a time table (UNGM dynamics), one without, and - for the measurement side's table, which no model pair of the
    // library has - the layout functions alone with a tabulated integrand in second place
    const int ids[3][2] = {{SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS}, {SSMQ_F_PENDULUM_DYN, SSMQ_F_PENDULUM_MEAS},
                           {SSMQ_F_PENDULUM_DYN, SSMQ_F_UNGMNA_DYN}};
    const int shapes[4][3] = {{1, 1, 1}, {1, 1, 5}, {5, 4, 3}, {6, 2, 0}};
    int cases = 0;
    for (const auto &id : ids)
        for (const auto &sh : shapes)
            for (int mask = 0; mask < 8; ++mask) {
                const int D = sh[0], Y = sh[1], T = sh[2];
                char what[96];
                snprintf(what, sizeof(what), "dyn %d obs %d D %d Y %d T %d inputs %d", id[0], id[1], D, Y, T, mask);
                ssmq_integrand fd = {}, fo = {};
                fd.id = id[0];
                fo.id = id[1];
                // exactly-sized heap inputs: an overrun of a read is the sanitizer's to report
                std::vector<double> gqg((size_t)D * D), rr((size_t)Y * Y), sc((size_t)T);
                for (size_t i = 0; i < gqg.size(); ++i) gqg[i] = 100.0 + (double)i;
                for (size_t i = 0; i < rr.size(); ++i) rr[i] = 200.0 + (double)i;
                for (size_t i = 0; i < sc.size(); ++i) sc[i] = 300.0 + (double)i;
                const double *GQG = (mask & 1) ? gqg.data() : nullptr, *R = (mask & 2) ? rr.data() : nullptr;
                // (a scale of T = 0 steps is an empty array, which is still "a scale was passed")
                static const double empty_scale[1] = {0.0};
                const double *S = (mask & 4) ? (T ? sc.data() : empty_scale) : nullptr;
                const size_t n = pass_consts_doubles(D, Y, T);
                CHECK(n % 8 == 0 && n >= (size_t)D * D + (size_t)Y * Y + 4 * (size_t)T && n < (size_t)D * D + (size_t)Y * Y + 4 * (size_t)T + 8);
                std::vector<double> img(n, -7.0);       // exactly n doubles: a write past the size is the sanitizer's to report
                const PassConsts c = fill_pass_consts(img.data(), &fd, &fo, D, Y, T, GQG, R, S);
                // the six segments in order, none overlapping, all inside the block
                const size_t start[7] = {0, c.rr, c.scale, c.ttab_dyn, c.ttab_obs, c.steps, c.steps + (size_t)T};
                const size_t len[6] = {(size_t)D * D, (size_t)Y * Y, (size_t)T, (size_t)T, (size_t)T, (size_t)T};
                for (int k = 0; k < 6; ++k) CHECK(start[k] + len[k] == start[k + 1]);
                CHECK(start[6] <= n);
                // contents
                for (size_t i = 0; i < len[0]; ++i) CHECK(img[i] == (GQG ? gqg[i] : 0.0));
                for (size_t i = 0; i < len[1]; ++i) CHECK(img[c.rr + i] == (R ? rr[i] : 0.0));
                const bool td = id[0] == SSMQ_F_UNGM_DYN && T > 0, to = id[1] == SSMQ_F_UNGMNA_DYN && T > 0;
                CHECK(td == (has_time_table(fd.id) && T > 0) && to == (has_time_table(fo.id) && T > 0));
                std::vector<double> ref((size_t)T + 1), ref_o((size_t)T + 1);
                if (td) CHECK(time_table(fd.id, T, ref.data()));
                if (to) CHECK(time_table(fo.id, T, ref_o.data()));
                for (int k = 0; k < T; ++k) {
                    CHECK(img[c.scale + k] == (S ? sc[k] : 1.0));
                    CHECK(img[c.ttab_dyn + k] == (td ? ref[k] : 0.0));
                    CHECK(img[c.ttab_obs + k] == (to ? ref_o[k] : 0.0));
                    CHECK(img[c.steps + k] == (double)k);
                }
                for (size_t i = start[6]; i < n; ++i) CHECK(img[i] == 0.0);
                CHECK(c.has_scale == (S != nullptr) && c.has_ttab_dyn == td && c.has_ttab_obs == to);
                // the pass's pointers: null exactly for an absent table and an absent scale
                std::vector<double> dev(n + 1);
                FilterPass p;
                wire_pass_consts(p, dev.data(), c);
                CHECK(p.gqg == dev.data() && p.rr == dev.data() + c.rr);
                CHECK(p.sscale == (S ? dev.data() + c.scale : nullptr));
                CHECK(p.ttab_dyn == (td ? dev.data() + c.ttab_dyn : nullptr));
                CHECK(p.ttab_obs == (to ? dev.data() + c.ttab_obs : nullptr));
                // a second fill of the same inputs is the same image (what the cached block's comparison relies on)
                std::vector<double> again(n, 9.0);
                fill_pass_consts(again.data(), &fd, &fo, D, Y, T, GQG, R, S);
                CHECK(again == img);
                ++cases;
            }
    if (g_failed) {
        printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("ok %d\n", cases);
    return 0;
}
