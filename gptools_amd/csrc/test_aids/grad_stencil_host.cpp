// grad_stencil_host.cpp -- test aid: the stencil builder and the launch-group walk of the differenced gradients (grad_stencil.inc, with
// api_kparams.inc for parse_model) as a stand-alone host program, built with the address and undefined-behaviour sanitizers
// (tests/test_grad_stencil_host.py).  No device code runs and no HIP call is made.  A few stencils through both: no entries, 11
// entries of one term (two groups: 8 + 3), interleaved terms of a three-term model with a product term, and the refusals.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <vector>
#include "../common.hpp"

static char g_err[512];
void gpt_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
#define GPT_TRY(expr)          \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != GPT_OK) return rc_; \
    } while (0)
#include "../api_kparams.inc"
#include "../grad_stencil.inc"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_err); \
            fails++;                                                     \
        }                                                                \
    } while (0)

struct Group { int b0, cnt, t; };
static std::vector<Group> groups_of(const GradStencil &s)
{
    std::vector<Group> g;
    for_each_group(s, [&](int b0, int cnt, int t) {
        g.push_back(Group{b0, cnt, t});
        return GPT_OK;
    });
    return g;
}

int main()
{
    const int D = 2;
    long colmax[GPT_MAX_DIM] = {0};
    // SE + Matern-5/2 * SE + general Matern at num_dim 2: 3, 6 and 4 parameters
    const int ids[3] = {GPT_KERNEL_SE, GPT_KERNEL_M52, GPT_KERNEL_MATERN}, ids2[3] = {-1, GPT_KERNEL_SE, -1};
    const int np[3] = {3, 6, 4}, np1[3] = {3, 3, 4};
    const double params[13] = {1.1, 0.4, 0.6, 0.7, 0.9, 1.3, 1.0, 1.5, 0.8, 1.0, 1.3, 0.35, 0.3};
    ModelKernel m;
    CHECK(parse_model(D, 0, colmax, 3, ids, ids2, params, np, np1, &m) == GPT_OK);
    {   // no entries: an empty stencil, no group
        GradStencil s;
        CHECK(grad_stencil_build("host", D, 0, colmax, m, 0, nullptr, nullptr, nullptr, nullptr, &s) == GPT_OK);
        CHECK(s.kp1.empty() && s.where.empty() && s.off.size() == 1 && groups_of(s).empty());
    }
    {   // 11 entries of term 1 (a product): two groups, 8 + 3; every stencil point carries its own first parameter
        const int nh = 11;
        std::vector<int> tix(nh, 1);
        std::vector<double> pa, pb, dn(nh, 1e-5);
        for (int h = 0; h < nh; h++)
            for (int q = 0; q < 6; q++) {
                pa.push_back(params[3 + q] + (q == 0 ? 0.01 * h : 0.0));
                pb.push_back(params[3 + q] + (q == 0 ? 0.01 * h + 1e-5 : 0.0));
            }
        GradStencil s;
        CHECK(grad_stencil_build("host", D, 0, colmax, m, nh, tix.data(), pa.data(), pb.data(), dn.data(), &s) == GPT_OK);
        CHECK(s.kp1.size() == 22 && s.kp2.size() == 22 && s.off[nh] == 66);
        const std::vector<Group> g = groups_of(s);
        CHECK(g.size() == 2 && g[0].b0 == 0 && g[0].cnt == 8 && g[1].b0 == 8 && g[1].cnt == 3 && g[0].t == 1 && g[1].t == 1);
        for (int h = 0; h < nh; h++) {
            CHECK(s.where[h] == h && s.kp1[2 * h].kernel_id == GPT_KERNEL_M52 && s.kp2[2 * h].kernel_id == GPT_KERNEL_SE);
            CHECK(s.kp1[2 * h].sigma == pa[6 * h] && s.kp1[2 * h + 1].sigma == pb[6 * h]);
        }
    }
    {   // interleaved terms: launch order is term by term, where[] leads back to the caller's entries
        const int tix[5] = {2, 0, 1, 0, 2};
        std::vector<double> pa, pb;
        const int start[3] = {0, 3, 9};
        for (int h = 0; h < 5; h++)
            for (int q = 0; q < np[tix[h]]; q++) {
                pa.push_back(params[start[tix[h]] + q]);
                pb.push_back(params[start[tix[h]] + q] * (1.0 + 1e-6));
            }
        const double dn[5] = {1e-6, -1e-6, 1e-6, 1e-6, 1e-6};
        GradStencil s;
        CHECK(grad_stencil_build("host", D, 0, colmax, m, 5, tix, pa.data(), pb.data(), dn, &s) == GPT_OK);
        const int want_where[5] = {1, 3, 2, 0, 4}, want_term[5] = {0, 0, 1, 2, 2};
        for (int i = 0; i < 5; i++) CHECK(s.where[i] == want_where[i] && s.term_of[i] == want_term[i]);
        CHECK(s.off[1] == 4 && s.off[2] == 7 && s.off[3] == 13 && s.off[4] == 16 && s.off[5] == 20);
        const std::vector<Group> g = groups_of(s);
        CHECK(g.size() == 3 && g[0].cnt == 2 && g[1].cnt == 1 && g[2].cnt == 2 && g[1].b0 == 2 && g[2].b0 == 3 && g[2].t == 2);
        CHECK(s.kp2[0].kernel_id < 0 && s.kp2[4].kernel_id == GPT_KERNEL_SE && s.kp1[6].kernel_id == GPT_KERNEL_MATERN);
        // the refusals, in the order the entry points have always given them
        GradStencil r;
        int bad_t[5] = {2, 0, 3, 0, 2};
        CHECK(grad_stencil_build("host", D, 0, colmax, m, 5, bad_t, pa.data(), pb.data(), dn, &r) == GPT_E_ARG);
        double bad_d[5] = {1e-6, 0.0, 1e-6, INFINITY, 1e-6};
        r = GradStencil();
        CHECK(grad_stencil_build("who", D, 0, colmax, m, 5, tix, pa.data(), pb.data(), bad_d, &r) == GPT_E_ARG && !strcmp(g_err, "who: denom[1] = 0"));
        bad_d[1] = 1e-6;
        r = GradStencil();
        CHECK(grad_stencil_build("who", D, 0, colmax, m, 5, tix, pa.data(), pb.data(), bad_d, &r) == GPT_E_ARG && !strcmp(g_err, "who: denom[3] = inf"));
        std::vector<double> nu = pb;
        nu[1] = 70.0;                      // entry 0 is the general Matern term: its nu
        r = GradStencil();
        CHECK(grad_stencil_build("who", D, 0, colmax, m, 5, tix, pa.data(), nu.data(), dn, &r) == GPT_E_VALUE && strstr(g_err, "nu") != nullptr);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
