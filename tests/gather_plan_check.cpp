// gather_plan_check.cpp -- csrc/gather_plan.h (the host side of eph_craft_batch_gather) against a naive model, on seeded random cases:
// 1-5 sources of 0-300 craft, with and without burns (1 to 7 timeline segments per craft), dealt (a random column permutation) and
// undealt, selections with duplicates, empty selections, concatenations, and every refusal. Checked: the merged CSR slice by slice,
// the per-source lists (output craft, source craft, source column), the depths, the flags. A stand-alone program (tests/
// test_gather_plan.py builds it with AddressSanitizer and UBSan); prints "cases N refusals M" and exits non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../ephemeris_explorer_amd/csrc/gather_plan.h"

struct Seg {
    double start, end, ax, ay, az;
    int is_burn, ref;
    bool operator==(const Seg &o) const {
        return start == o.start && end == o.end && ax == o.ax && ay == o.ay && az == o.az && is_burn == o.is_burn && ref == o.ref;
    }
};
using Source = eph::GatherSource<Seg>;
using Plan = eph::GatherPlan<Seg>;

struct Batch {                       // what a source batch holds on the host
    long long n = 0;
    int max_knots = 1, max_tr = 0, max_ap = 0;
    std::vector<int> slot;
    std::vector<long long> seg_off;
    std::vector<Seg> segs;
    std::vector<int32_t> body_order;
    std::vector<double> soi;
    unsigned char method[24] = {};
    eph_adaptive_params params{};
    int pv = 0;
    bool retry = false, events = false;
    int ephemeris = 0;
};

static std::mt19937_64 rng(20261019);
static long long uniform(long long lo, long long hi) { return std::uniform_int_distribution<long long>(lo, hi)(rng); }

static void fail(const std::string &what, long long c) {
    std::printf("MISMATCH in case %lld: %s\n", c, what.c_str());
    std::exit(1);
}

static Batch random_batch(bool burns, bool events, long long serial) {
    Batch b;
    b.n = uniform(0, 3) == 0 ? uniform(0, 2) : uniform(0, 300);
    b.max_knots = (int)uniform(1, 500);
    b.events = events;
    if (events) { b.max_tr = (int)uniform(3, 64); b.max_ap = (int)uniform(3, 1024); b.soi = {1.0, 2.0, INFINITY}; }
    if (b.n >= 128 && uniform(0, 1)) {
        b.slot.resize((size_t)b.n);
        for (long long i = 0; i < b.n; ++i) b.slot[(size_t)i] = (int)i;
        std::shuffle(b.slot.begin(), b.slot.end(), rng);
    }
    b.seg_off.assign((size_t)b.n + 1, 0);
    for (long long i = 0; i < b.n; ++i) {
        const long long nseg = burns ? 1 + 2 * uniform(0, 3) : 1;
        for (long long k = 0; k < nseg; ++k)
            b.segs.push_back(Seg{(double)serial, (double)i, (double)k, 0.5 * (double)uniform(0, 1000), -1.0, (int)(k & 1), (int)uniform(-1, 4)});
        b.seg_off[(size_t)i + 1] = (long long)b.segs.size();
    }
    for (unsigned char &m : b.method) m = 7;
    b.params.h_init = 60.0; b.params.h_max = 1e9; b.params.tol_position = 1e-3; b.params.tol_velocity = 1e-3;
    b.params.fac_min = 0.2; b.params.fac_max = 5.0; b.params.fac = 0.9; b.params.n_max = 1000;
    return b;
}
static std::vector<Source> describe(const std::vector<Batch> &bs, const int *ephemeris) {
    std::vector<Source> out;
    for (const Batch &b : bs) {
        Source g;
        g.ephemeris = ephemeris + b.ephemeris; g.method = b.method; g.method_bytes = sizeof(b.method); g.params = b.params;
        g.pair_variant = b.pv; g.body_order = &b.body_order; g.retry = b.retry; g.events = b.events; g.soi = b.events ? &b.soi : nullptr;
        g.n = b.n; g.max_knots = b.max_knots; g.max_tr = b.max_tr; g.max_ap = b.max_ap;
        g.slot = &b.slot; g.seg_off = &b.seg_off; g.segs = &b.segs;
        out.push_back(g);
    }
    return out;
}

int main() {
    static const int ephemeris[2] = {0, 0};
    long long cases = 0, refusals = 0, dealt_sources = 0, duplicates = 0, empty = 0, with_burns = 0;
    for (long long c = 0; c < 3000; ++c) {
        const bool burns = uniform(0, 1), events = uniform(0, 1);
        const int ns = (int)uniform(1, 5);
        std::vector<Batch> bs;
        long long total = 0;
        for (int s = 0; s < ns; ++s) { bs.push_back(random_batch(burns, events, c * 8 + s)); total += bs.back().n; dealt_sources += !bs.back().slot.empty(); }
        with_burns += burns;
        // the selection: a concatenation, one source's craft, or craft of all sources
        const int kind = (int)uniform(0, 2);
        std::vector<int32_t> source_of;
        std::vector<int64_t> craft_of;
        long long n_out = total;
        if (kind != 0) {
            n_out = uniform(0, 4) == 0 ? 0 : uniform(0, 400);
            std::vector<int> usable;
            for (int s = 0; s < (kind == 1 ? 1 : ns); ++s) if (bs[(size_t)s].n > 0) usable.push_back(s);
            if (usable.empty()) n_out = 0;
            for (long long i = 0; i < n_out; ++i) {
                const int s = usable[(size_t)uniform(0, (long long)usable.size() - 1)];
                source_of.push_back(s);
                craft_of.push_back(i > 0 && uniform(0, 9) == 0 && source_of[(size_t)i - 1] == s ? craft_of[(size_t)i - 1] : uniform(0, bs[(size_t)s].n - 1));
                duplicates += i > 0 && craft_of[(size_t)i] == craft_of[(size_t)i - 1] && source_of[(size_t)i - 1] == s;
            }
            source_of.resize((size_t)n_out + 1, 0);           // (never empty: data() of an empty selection is still a pointer)
            craft_of.resize((size_t)n_out + 1, 0);
        }
        empty += n_out == 0;
        const bool one = kind == 1 && ns == 1;                // source_of == NULL is allowed with a single source only
        const int32_t *so = kind == 0 || one ? nullptr : source_of.data();
        const int64_t *co = kind == 0 ? nullptr : craft_of.data();
        // ---- refusals: one disagreement or one bad argument at a time ----
        if (ns > 1) {
            const int which = (int)uniform(0, 8), s = (int)uniform(1, ns - 1);
            std::vector<Batch> bad = bs;
            const char *want = "";
            switch (which) {
            case 0: bad[(size_t)s].ephemeris = 1; want = "ephemeris"; break;
            case 1: bad[(size_t)s].method[5] ^= 1; want = "method"; break;
            case 2: reinterpret_cast<unsigned char *>(&bad[(size_t)s].params)[uniform(0, 59)] ^= 0x10; want = "adaptive parameters"; break;
            case 3: bad[(size_t)s].pv = 3; want = "evaluation order"; break;
            case 4: bad[(size_t)s].body_order = {1, 0, 2}; want = "body order"; break;
            case 5: bad[(size_t)s].retry = true; want = "retry_failed"; break;
            case 6: bad[(size_t)s].events = !events; bad[(size_t)s].soi = {1.0, 2.0, INFINITY}; want = "events on / off"; break;
            case 7: if (events) { bad[(size_t)s].soi[1] = 2.0000000000000004; want = "soi radii"; } else { bad[(size_t)s].pv = 1; want = "evaluation order"; } break;
            default: bad[0].retry = true; want = "retry_failed"; break;
            }
            const Plan p = eph::gather_plan(describe(bad, ephemeris), n_out, so, co);
            if (p.status != EPH_ERR_BAD_ARGUMENT || p.error.find(want) == std::string::npos || !p.items.empty() || !p.segs.empty())
                fail(std::string("a disagreement in ") + want + " was not refused: " + p.error, c);
            // the FIRST disagreement is named: the lowest such source
            if (which != 8 && p.error.find("source " + std::to_string(s) + " ") == std::string::npos) fail("wrong source named: " + p.error, c);
            ++refusals;
        }
        {
            const std::vector<Source> d = describe(bs, ephemeris);
            auto refused = [&](const Plan &p, const char *what) {
                if (p.status != EPH_ERR_BAD_ARGUMENT || p.error.empty() || !p.items.empty() || !p.seg_off.empty()) fail(what, c);
                ++refusals;
            };
            refused(eph::gather_plan(d, -1, so, co), "n_out < 0");
            refused(eph::gather_plan(std::vector<Source>{}, n_out, so, co), "no sources");
            if (ns > 1) refused(eph::gather_plan(d, n_out, nullptr, craft_of.empty() ? reinterpret_cast<const int64_t *>(&c) : craft_of.data()), "source_of NULL with several sources");
            refused(eph::gather_plan(d, n_out, source_of.empty() ? reinterpret_cast<const int32_t *>(&c) : source_of.data(), nullptr), "craft_of NULL with source_of");
            refused(eph::gather_plan(d, total + 1, nullptr, nullptr), "a concatenation of another size");
            if (kind != 0 && n_out > 0) {
                std::vector<int64_t> off = craft_of;
                const size_t i = (size_t)uniform(0, n_out - 1);
                off[i] = uniform(0, 1) ? -1 : bs[(size_t)(so ? source_of[i] : 0)].n;
                refused(eph::gather_plan(d, n_out, so, off.data()), "a craft index outside its source");
                if (so) {
                    std::vector<int32_t> os = source_of;
                    os[i] = uniform(0, 1) ? -1 : ns;
                    refused(eph::gather_plan(d, n_out, os.data(), co), "a source index outside the sources");
                }
            }
            const void *handles[5] = {&bs, &bs, &bs, &bs, &bs};
            std::string text;
            if (eph::gather_check_arguments(ns, handles, n_out, so, co, &text, text) != EPH_OK) fail("good arguments refused: " + text, c);
            if (eph::gather_check_arguments(ns, handles, n_out, so, co, nullptr, text) == EPH_OK || eph::gather_check_arguments(0, handles, n_out, so, co, &text, text) == EPH_OK ||
                eph::gather_check_arguments(ns, nullptr, n_out, so, co, &text, text) == EPH_OK || eph::gather_check_arguments(ns, handles, -1, so, co, &text, text) == EPH_OK)
                fail("bad arguments accepted", c);
            handles[ns - 1] = nullptr;
            if (eph::gather_check_arguments(ns, handles, n_out, so, co, &text, text) == EPH_OK) fail("a NULL source accepted", c);
            refusals += 5;
        }
        // ---- the plan against the model ----
        const Plan p = eph::gather_plan(describe(bs, ephemeris), n_out, so, co);
        if (p.status != EPH_OK || !p.error.empty()) fail("refused: " + p.error, c);
        int mk = 0, mt = 0, ma = 0;
        for (const Batch &b : bs) { mk = std::max(mk, b.max_knots); mt = std::max(mt, b.max_tr); ma = std::max(ma, b.max_ap); }
        if (p.n_out != n_out || p.max_knots != mk || p.max_tr != (events ? mt : 0) || p.max_ap != (events ? ma : 0) || p.events != events || p.retry)
            fail("depths or flags", c);
        if ((long long)p.seg_off.size() != n_out + 1 || (int)p.items.size() != ns || p.seg_off[0] != 0 || p.seg_off[(size_t)n_out] != (long long)p.segs.size())
            fail("shape", c);
        std::vector<size_t> cursor((size_t)ns, 0);
        long long concat_source = 0, concat_first = 0;
        for (long long i = 0; i < n_out; ++i) {
            long long s, k;
            if (kind == 0) {
                while (i - concat_first >= bs[(size_t)concat_source].n) { concat_first += bs[(size_t)concat_source].n; ++concat_source; }
                s = concat_source; k = i - concat_first;
            } else { s = so ? source_of[(size_t)i] : 0; k = craft_of[(size_t)i]; }
            const Batch &b = bs[(size_t)s];
            if (cursor[(size_t)s] >= p.items[(size_t)s].size()) fail("a source's list is short", c);
            const eph::GatherItem it = p.items[(size_t)s][cursor[(size_t)s]++];
            if (it.out != i || it.craft != k || it.col != (b.slot.empty() ? k : (long long)b.slot[(size_t)k])) fail("a list entry", c);
            const long long s0 = b.seg_off[(size_t)k], s1 = b.seg_off[(size_t)k + 1], o0 = p.seg_off[(size_t)i], o1 = p.seg_off[(size_t)i + 1];
            if (o1 - o0 != s1 - s0 || o0 < 0 || o1 > (long long)p.segs.size()) fail("a slice's length", c);
            for (long long q = 0; q < s1 - s0; ++q)
                if (!(p.segs[(size_t)(o0 + q)] == b.segs[(size_t)(s0 + q)])) fail("a slice's segment", c);
        }
        for (int s = 0; s < ns; ++s)
            if (cursor[(size_t)s] != p.items[(size_t)s].size()) fail("a source's list is long", c);
        ++cases;
    }
    std::printf("cases %lld refusals %lld dealt_sources %lld duplicates %lld empty %lld with_burns %lld\n", cases, refusals, dealt_sources, duplicates,
                empty, with_burns);
    return 0;
}
