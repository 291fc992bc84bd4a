// Host check of csrc/nlm_vbox_plan.hpp, the plan of the NLM strip kernel's vertical patch sums (built and run by test_vbox_plan.py).
// The planned additions are carried out in float on small integer-valued rows, where every order of additions is exact, for patch
// widths 1..16, strips of 4 and 8 rows, the whole strip and both of its halves.
#include "../image_denoising_filter_amd/csrc/nlm_vbox_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mid;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// One operation of the plan.  kind 'S' / 'P': row m's step of a running sum, continued from row `from` (-1: the sum starts at m),
// folded into the squared-difference FMAs or not.  kind 'V': output m from S[m] (a) and / or Pf[m+PW-1] (b).
struct Op {
    char kind; int m, from; bool folded, a, b;
    bool operator==(const Op &o) const { return kind == o.kind && m == o.m && from == o.from && folded == o.folded && a == o.a && b == o.b; }
};

static std::vector<Op> ops_of(const VboxPlan &p)
{
    const VboxOrder o = vbox_order(p);
    std::vector<Op> ops;
    for (int i = 0; i < o.count; ++i) {
        const VboxRow &r = p.row[o.row[i]];
        ops.push_back(Op{o.is_s[i] ? 'S' : 'P', o.row[i], o.is_s[i] ? r.s_from : r.p_from, r.single, false, false});
    }
    for (int k = p.k0; k < p.k1; ++k) ops.push_back(Op{'V', k, -1, false, p.v_uses_s(k), p.v_uses_p(k)});
    return ops;
}

// Carries the operations out the way the kernel does: a folded row adds its distance onto the sum it continues, any other row is
// formed once (at its first appearance) and added.  Uses only rows [p.lo, p.hi) and only values that were produced before.
static void evaluate(const VboxPlan &p, const float *rows, float *V)
{
    const VboxOrder o = vbox_order(p);
    std::vector<float> S(p.n, 0.f), Pf(p.n, 0.f), D(p.n, 0.f);
    std::vector<char> hasS(p.n, 0), hasP(p.n, 0), hasD(p.n, 0);
    for (int i = 0; i < o.count; ++i) {
        const int m = o.row[i];
        const VboxRow &r = p.row[m];
        CHECK(m >= p.lo && m < p.hi, "pw %d rs %d [%d,%d): row %d outside the rows the outputs read", p.pw, p.rs, p.k0, p.k1, m);
        CHECK(o.first[i] == !hasD[m], "pw %d rs %d: first flag of row %d", p.pw, p.rs, m);
        CHECK(o.is_s[i] ? r.s_live : r.p_live, "pw %d rs %d: dead sum of row %d issued", p.pw, p.rs, m);
        const int from = o.is_s[i] ? r.s_from : r.p_from;
        float prev = 0.f;
        if (from >= 0) {
            CHECK(from == (o.is_s[i] ? m + 1 : m - 1), "pw %d rs %d: row %d continues row %d", p.pw, p.rs, m, from);
            CHECK(o.is_s[i] ? hasS[from] : hasP[from], "pw %d rs %d: row %d uses the sum of row %d before it exists", p.pw, p.rs, m, from);
            prev = o.is_s[i] ? S[from] : Pf[from];
        }
        float v;
        if (r.single) {
            CHECK(from >= 0 && r.s_live != r.p_live, "pw %d rs %d: row %d is not single-use", p.pw, p.rs, m);
            CHECK(!hasD[m], "pw %d rs %d: folded row %d issued twice", p.pw, p.rs, m);
            v = rows[m] + prev;
        } else {
            if (!hasD[m]) { D[m] = rows[m]; hasD[m] = 1; }
            v = from >= 0 ? D[m] + prev : D[m];
        }
        hasD[m] = 1;
        if (o.is_s[i]) { S[m] = v; hasS[m] = 1; } else { Pf[m] = v; hasP[m] = 1; }
    }
    for (int k = p.k0; k < p.k1; ++k) {
        float v = 0.f;
        if (p.v_uses_s(k)) { CHECK(hasS[k], "pw %d rs %d: V[%d] needs S[%d]", p.pw, p.rs, k, k); v += S[k]; }
        if (p.v_uses_p(k)) { CHECK(hasP[k + p.pw - 1], "pw %d rs %d: V[%d] needs Pf[%d]", p.pw, p.rs, k, k + p.pw - 1); v += Pf[k + p.pw - 1]; }
        V[k] = v;
    }
}

static bool subsequence(const std::vector<Op> &half, const std::vector<Op> &full, char kind)
{
    size_t j = 0;
    for (const Op &h : half) {
        if (h.kind != kind) continue;
        while (j < full.size() && !(full[j] == h)) ++j;
        if (j == full.size()) return false;
        ++j;
    }
    return true;
}

// the operations of `full` that the outputs [k0, k1) depend on
static size_t needed(const VboxPlan &full, int k0, int k1)
{
    std::vector<char> s(full.n, 0), f(full.n, 0);
    for (int k = k0; k < k1; ++k) {
        if (full.v_uses_s(k)) for (int m = k; m >= 0 && !s[m]; m = full.row[m].s_from) s[m] = 1;
        if (full.v_uses_p(k)) for (int m = k + full.pw - 1; m >= 0 && !f[m]; m = full.row[m].p_from) f[m] = 1;
    }
    size_t c = (size_t)(k1 - k0);
    for (int m = 0; m < full.n; ++m) c += s[m] + f[m];
    return c;
}

// the plan must be usable in constant expressions: that is how the kernels read it
static_assert(vbox_plan(7, 8, 0, 8).folded == 12, "7x7 patch, strips of eight rows: twelve of the fourteen rows fold");
static_assert(VboxPlanOf<7, 8, 0, 4>::plan.folded == 8 && VboxPlanOf<7, 8, 4, 8>::plan.folded == 8, "the halves of that strip");
static_assert(VboxPlanOf<7, 8, 0, 8>::order.count == 14, "one step per row");

int main()
{
    for (int rs : {4, 8}) {
        for (int pw = 1; pw <= 16; ++pw) {
            const int n = rs + pw - 1;
            std::vector<float> rows(n);
            for (int m = 0; m < n; ++m) rows[m] = (float)((m * 7 + pw * 3 + rs) % 11 + 1);     // small integers: every sum is exact
            const VboxPlan full = vbox_plan(pw, rs, 0, rs);
            const std::vector<Op> full_ops = ops_of(full);
            const int ranges[3][2] = {{0, rs}, {0, rs / 2}, {rs / 2, rs}};
            for (const auto &rg : ranges) {
                const VboxPlan p = vbox_plan(pw, rs, rg[0], rg[1]);
                CHECK(p.n == n && p.lo == rg[0] && p.hi == rg[1] + pw - 1, "pw %d rs %d: extent", pw, rs);
                std::vector<float> V(rs, -1.f);
                evaluate(p, rows.data(), V.data());
                for (int k = rg[0]; k < rg[1]; ++k) {
                    float want = 0.f;
                    for (int i = 0; i < pw; ++i) want += rows[k + i];
                    CHECK(V[k] == want, "pw %d rs %d [%d,%d): V[%d] = %g, box sum %g", pw, rs, rg[0], rg[1], k, V[k], want);
                }
                // a sub-range performs the whole strip's operations for its outputs: the same operands, per running-sum kind in
                // the same order, none missing and none extra -- hence the same bits
                const std::vector<Op> ops = ops_of(p);
                for (const Op &h : ops) {
                    bool found = false;
                    for (const Op &f : full_ops) found = found || f == h;
                    CHECK(found, "pw %d rs %d [%d,%d): %c[%d] from %d folded %d is no operation of the whole strip", pw, rs, rg[0], rg[1], h.kind, h.m, h.from, (int)h.folded);
                }
                for (char kind : {'S', 'P', 'V'})
                    CHECK(subsequence(ops, full_ops, kind), "pw %d rs %d [%d,%d): %c operations are no sub-list of the whole strip's", pw, rs, rg[0], rg[1], kind);
                CHECK(ops.size() == needed(full, rg[0], rg[1]), "pw %d rs %d [%d,%d): %zu operations, the outputs need %zu", pw, rs, rg[0], rg[1], ops.size(), needed(full, rg[0], rg[1]));
                int folded = 0;
                for (const Op &h : ops) folded += (h.kind != 'V' && h.folded) ? 1 : 0;
                CHECK(folded == p.folded, "pw %d rs %d: folded count", pw, rs);
            }
        }
    }
    // Folded rows, counted by hand.  A row folds when exactly one running sum uses it and that sum does not start there.
    struct { int pw, rs, k0, k1, folded; const char *why; } hand[] = {
        {7, 8, 0, 8, 12, "blocks [0-6][7-13]: S runs 6->0, Pf runs 7->13; all rows but the two first rows 6 and 7"},
        {7, 8, 0, 4, 8, "upper half: S 6->0 folds rows 0-5, Pf 7->9 folds rows 8, 9"},
        {7, 8, 4, 8, 8, "lower half: S 6->4 folds rows 4, 5, Pf 7->13 folds rows 8-13"},
        {7, 4, 0, 4, 8, "a four-row strip is the upper half of the eight-row one"},
        {1, 8, 0, 8, 0, "1x1 patch: every row is a block of its own, every sum starts where it ends"},
        {3, 8, 0, 8, 2, "blocks [0-2][3-5][6-8][9]: rows 0, 1 fold into S 2->0; rows 3, 6, 9 start a Pf, rows 4, 5, 7, 8 are in S and Pf"},
        {6, 8, 0, 8, 5, "blocks [0-5][6-11][12]: rows 0-4 fold into S 5->0; rows 6, 12 start a Pf, rows 7-11 are in S (for V[7]) and Pf"},
        {8, 8, 0, 8, 13, "blocks [0-7][8-14]: S 7->0 folds rows 0-6, Pf 8->14 folds rows 9-14"},
        {9, 8, 0, 8, 14, "blocks [0-8][9-15]: S 8->0 folds rows 0-7, Pf 9->15 folds rows 10-15"},
        {16, 4, 0, 4, 17, "blocks [0-15][16-18]: S 15->0 folds rows 0-14, Pf 16->18 folds rows 17, 18"},
    };
    for (const auto &c : hand) {
        const VboxPlan p = vbox_plan(c.pw, c.rs, c.k0, c.k1);
        CHECK(p.folded == c.folded, "pw %d rs %d [%d,%d): %d rows fold, by hand %d (%s)", c.pw, c.rs, c.k0, c.k1, p.folded, c.folded, c.why);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("vbox plan: all checks passed\n");
    return 0;
}
