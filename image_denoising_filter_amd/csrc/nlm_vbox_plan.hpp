// nlm_vbox_plan.hpp -- the compile-time plan of the NLM strip kernel's vertical patch sums (nlm_strip.hpp).  Plain C++, no HIP: the
// kernels evaluate it in `if`s that fold away after unrolling, tests/vbox_plan_host.cpp evaluates it on the host.
//
// V[k] = D[k] + ... + D[k+PW-1] for the output rows k of a strip of RS rows, with the block decomposition of van Herk / Gil-Werman
// (vertical_box, nlm_strip.hpp): the RS + PW - 1 distance rows are cut into blocks of PW, S[m] is the running sum from row m to the end
// of its block, Pf[m] the one from the start of its block to row m, and
//     V[0] = S[0],   V[k] = Pf[k+PW-1] where k starts a block,   V[k] = S[k] + Pf[k+PW-1] otherwise.
// The plan says which of those running sums the REQUESTED output rows [k0, k1) need -- nothing else is live -- and which rows are
// *single-use*: live in exactly one running sum of the whole strip and not that sum's first row.  Such a row's squared differences can be accumulated
// straight onto the running sum, S[m] = fma(dz,dz, fma(dy,dy, fma(dx,dx, S[m+1]))), which saves the separate addition (and one
// rounding).  Every other live row -- the first row of a running sum, or a row that two running sums share (strips taller than PW + 1)
// -- is formed on its own, D[m], and added.  Liveness starts from the outputs alone, so a wave that takes half of a strip (the HALF
// launch shape: [0, 4) or [4, 8) of RS = 8) performs exactly the operations the whole strip performs for those outputs, operands and
// order included: the plan of a sub-range is a sub-list of the full plan, and the bits are the same.
#pragma once

namespace mid {

constexpr int kVboxMaxRows = 32;   // RS + PW - 1 <= 8 + 16 - 1

struct VboxRow {
    bool s_live, p_live;   // S[m] / Pf[m] feeds one of the requested outputs
    int s_from, p_from;    // the row whose running sum this one continues (m + 1 / m - 1), or -1: the sum starts here
    bool single;           // live in exactly one running sum and not its first row: folded into the squared-difference FMAs
};

struct VboxPlan {
    int pw, rs, k0, k1;    // what was asked (the kernels read n, folded, row[] and v_uses_*; the rest is for tests/vbox_plan_host.cpp)
    int n;                 // RS + PW - 1 distance rows in the strip's frame
    int lo, hi;            // the rows [lo, hi) the outputs [k0, k1) read: k0 .. k1 + PW - 2
    int folded;            // number of single-use rows
    VboxRow row[kVboxMaxRows];
    // how output k is formed: from S[k] alone, from Pf[k+PW-1] alone, or from their sum
    constexpr bool v_uses_s(int k) const { return k == 0 || k % pw != 0; }
    constexpr bool v_uses_p(int k) const { return k != 0; }
};

constexpr VboxPlan vbox_plan(int pw, int rs, int k0, int k1)
{
    VboxPlan p{};
    p.pw = pw; p.rs = rs; p.k0 = k0; p.k1 = k1;
    p.n = rs + pw - 1;
    p.lo = k0; p.hi = k1 + pw - 1;
    for (int m = 0; m < kVboxMaxRows; ++m) p.row[m] = VboxRow{false, false, -1, -1, false};
    for (int k = k0; k < k1; ++k) {
        if (p.v_uses_s(k)) p.row[k].s_live = true;
        if (p.v_uses_p(k)) p.row[k + pw - 1].p_live = true;
    }
    // S runs towards lower rows, Pf towards higher rows: a live sum keeps the sum it continues alive
    for (int m = 0; m < p.n; ++m) {
        const bool block_end = (m % pw == pw - 1) || (m == p.n - 1);
        if (p.row[m].s_live && !block_end) { p.row[m].s_from = m + 1; p.row[m + 1].s_live = true; }
    }
    for (int m = p.n - 1; m >= 0; --m) {
        const bool block_start = (m % pw == 0);
        if (p.row[m].p_live && !block_start) { p.row[m].p_from = m - 1; p.row[m - 1].p_live = true; }
    }
    // Single-use is a property of the WHOLE strip's sums: a row that two sums of the strip share is formed on its own in a half
    // too, even where the half needs only one of the two (6x6 patch, row 7: S for V[7], Pf for V[2]) -- else the half would round
    // that row differently from the whole strip.
    if (k0 != 0 || k1 != rs) {
        const VboxPlan whole = vbox_plan(pw, rs, 0, rs);
        for (int m = 0; m < p.n; ++m) p.row[m].single = whole.row[m].single && (p.row[m].s_live || p.row[m].p_live);
    } else {
        for (int m = 0; m < p.n; ++m) {
            const VboxRow &r = p.row[m];
            p.row[m].single = (r.s_live != r.p_live) && (r.s_live ? r.s_from >= 0 : r.p_from >= 0);
        }
    }
    for (int m = 0; m < p.n; ++m) p.folded += p.row[m].single ? 1 : 0;
    return p;
}

// The order the running sums are issued in: the S rows from the highest down and the Pf rows from the lowest up, ALTERNATED row by
// row, so that consecutive dependent FMAs belong to different chains (the compiler's scheduler arrives at the same interleaving from
// other source orders too: tools/experiments/README.md).  slot i of the order: row[i], and whether it is the row's S
// (true) or Pf (false) step; count entries.  A row live in both sums appears twice: its D[m] is formed at the first appearance (first).
struct VboxOrder {
    int count;
    int row[2 * kVboxMaxRows];
    bool is_s[2 * kVboxMaxRows];
    bool first[2 * kVboxMaxRows];
};

constexpr VboxOrder vbox_order(const VboxPlan &p)
{
    VboxOrder o{};
    bool seen[kVboxMaxRows] = {};
    int s = p.n - 1, f = 0;
    while (s >= 0 || f < p.n) {
        while (s >= 0 && !p.row[s].s_live) --s;
        if (s >= 0) { o.row[o.count] = s; o.is_s[o.count] = true; o.first[o.count] = !seen[s]; seen[s] = true; ++o.count; --s; }
        while (f < p.n && !p.row[f].p_live) ++f;
        if (f < p.n) { o.row[o.count] = f; o.is_s[o.count] = false; o.first[o.count] = !seen[f]; seen[f] = true; ++o.count; ++f; }
    }
    return o;
}

template <int PW, int RS, int K0, int K1>
struct VboxPlanOf {
    static constexpr VboxPlan plan = vbox_plan(PW, RS, K0, K1);
    static constexpr VboxOrder order = vbox_order(plan);
};

}  // namespace mid
