// gather_plan.h -- the host side of eph_craft_batch_gather (craft_gather.hip) as a pure host value, in the manner of table_layout.h:
// the argument and agreement checks, for each source the list of (output craft, source craft, source column), the merged timeline
// CSR built from the sources' host mirrors, and the output's depths. No device, no handle: the call describes its sources as
// GatherSource values, the plan only does arithmetic. Plain C++ (tests/gather_plan_check.cpp compiles this header alone); the
// segment type is a template parameter because SegmentDev lives in a device header.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ephemeris_amd.h"

namespace eph {

// what the plan needs to know of one source batch
template <class Seg>
struct GatherSource {
    const void *ephemeris = nullptr;              // the eph_ephemeris handle (and with it the device)
    const void *method = nullptr;                 // the coefficient table's bytes (one table per ErkCoeffs name)
    size_t method_bytes = 0;
    eph_adaptive_params params{};
    int pair_variant = 0;                         // evaluation order of the point-mass term
    const std::vector<int32_t> *body_order = nullptr;
    bool retry = false, events = false;
    const std::vector<double> *soi = nullptr;     // events on: the sphere radii (null: not compared; the call compares them once it
                                                  //   has read them from the device, through gather_soi_agree)
    long long n = 0;
    int max_knots = 0, max_tr = 0, max_ap = 0;
    const std::vector<int> *slot = nullptr;       // craft -> knot slab column (null or empty: undealt, column = craft)
    const std::vector<long long> *seg_off = nullptr;   // the timeline CSR's host mirror: n + 1 offsets into segs
    const std::vector<Seg> *segs = nullptr;
};
struct GatherItem {
    long long out, craft, col;                    // output craft <- craft `craft` of the source, whose knots lie in column `col`
};
template <class Seg>
struct GatherPlan {
    int status = EPH_OK;                          // EPH_ERR_BAD_ARGUMENT: `error` names the first disagreement, the rest is empty
    std::string error;
    long long n_out = 0;
    int max_knots = 0, max_tr = 0, max_ap = 0;
    bool events = false, retry = false;
    std::vector<std::vector<GatherItem>> items;   // per source, in output order
    std::vector<long long> seg_off;               // n_out + 1; craft i's segments are segs[seg_off[i] .. seg_off[i + 1]), a craft's
    std::vector<Seg> segs;                        //   current segment stays RELATIVE to its slice
};

// the rules on the counts and the NULL combinations, stated once: the text of the first one broken, or nullptr
inline const char *gather_shape_error(long long n_sources, long long n_out, const int32_t *source_of, const int64_t *craft_of) {
    if (n_sources < 1) return "gather: n_sources < 1";
    if (n_out < 0) return "gather: n_out < 0";
    if (!source_of && craft_of && n_sources != 1) return "gather: source_of == NULL needs n_sources == 1";
    if (source_of && !craft_of) return "gather: craft_of == NULL needs source_of == NULL";
    return nullptr;
}

// the argument rules that need no source: EPH_ERR_BAD_ARGUMENT and a text, or EPH_OK
inline int gather_check_arguments(int n_sources, const void *const *sources, long long n_out, const int32_t *source_of,
                                  const int64_t *craft_of, const void *out, std::string &error) {
    if (!out) { error = "gather: out is NULL"; return EPH_ERR_BAD_ARGUMENT; }
    if (const char *text = gather_shape_error(n_sources, n_out, source_of, craft_of)) { error = text; return EPH_ERR_BAD_ARGUMENT; }
    if (!sources) { error = "gather: sources is NULL"; return EPH_ERR_BAD_ARGUMENT; }
    for (int s = 0; s < n_sources; ++s)            // (last: the rules above are decided without looking at a source)
        if (!sources[s]) { error = "gather: source " + std::to_string(s) + " is NULL"; return EPH_ERR_BAD_ARGUMENT; }
    return EPH_OK;
}

// bytewise-equal sphere radii (events on): the first source that differs from source 0, or -1
inline int gather_soi_agree(const std::vector<const std::vector<double> *> &soi) {
    for (size_t s = 1; s < soi.size(); ++s)
        if (soi[s]->size() != soi[0]->size() ||
            (!soi[0]->empty() && std::memcmp(soi[s]->data(), soi[0]->data(), sizeof(double) * soi[0]->size()) != 0))
            return (int)s;
    return -1;
}

template <class Seg>
GatherPlan<Seg> gather_plan(const std::vector<GatherSource<Seg>> &src, long long n_out, const int32_t *source_of,
                            const int64_t *craft_of) {
    GatherPlan<Seg> plan;
    auto refuse = [&plan](const std::string &text) {
        GatherPlan<Seg> bad;
        bad.status = EPH_ERR_BAD_ARGUMENT;
        bad.error = text;
        plan = std::move(bad);
        return plan;
    };
    const int ns = (int)src.size();
    if (const char *text = gather_shape_error(ns, n_out, source_of, craft_of)) return refuse(text);
    // the sources agree with source 0
    const GatherSource<Seg> &a = src[0];
    for (int s = 1; s < ns; ++s) {
        const GatherSource<Seg> &b = src[(size_t)s];
        const std::string who = "gather: source " + std::to_string(s) + " differs from source 0 in ";
        if (b.ephemeris != a.ephemeris) return refuse(who + "its ephemeris");
        if (b.method_bytes != a.method_bytes || (a.method_bytes && std::memcmp(b.method, a.method, a.method_bytes) != 0))
            return refuse(who + "its method");
        // (the bytes of the fields: the structure's tail padding is nobody's to compare)
        if (std::memcmp(&b.params, &a.params, offsetof(eph_adaptive_params, n_max) + sizeof(a.params.n_max)) != 0)
            return refuse(who + "its adaptive parameters");
        if (b.pair_variant != a.pair_variant) return refuse(who + "the evaluation order of the point-mass term");
        static const std::vector<int32_t> table_order;
        const std::vector<int32_t> &oa = a.body_order ? *a.body_order : table_order, &ob = b.body_order ? *b.body_order : table_order;
        if (oa != ob) return refuse(who + "its body order");
        if (b.retry != a.retry) return refuse(who + "a pending retry_failed");
        if (b.events != a.events) return refuse(who + "events on / off");
        if (a.events && a.soi && b.soi) {
            const std::vector<const std::vector<double> *> two{a.soi, b.soi};
            if (gather_soi_agree(two) >= 0) return refuse(who + "its soi radii");
        }
    }
    // the selection
    long long total = 0;
    for (const GatherSource<Seg> &g : src) total += g.n;
    if (!craft_of && n_out != total) return refuse("gather: craft_of == NULL needs n_out == the sum of the sources' sizes");
    for (long long i = 0; craft_of && i < n_out; ++i) {
        const long long s = source_of ? source_of[i] : 0;
        if (s < 0 || s >= ns) return refuse("gather: source_of[" + std::to_string(i) + "] is outside the sources");
        if (craft_of[i] < 0 || craft_of[i] >= src[(size_t)s].n)
            return refuse("gather: craft_of[" + std::to_string(i) + "] is outside source " + std::to_string(s));
    }
    plan.n_out = n_out;
    plan.events = a.events;
    plan.retry = a.retry;
    for (const GatherSource<Seg> &g : src) {
        plan.max_knots = std::max(plan.max_knots, g.max_knots);
        if (a.events) { plan.max_tr = std::max(plan.max_tr, g.max_tr); plan.max_ap = std::max(plan.max_ap, g.max_ap); }
    }
    plan.items.assign((size_t)ns, {});
    plan.seg_off.assign((size_t)n_out + 1, 0);
    long long first = 0;                          // craft_of == NULL: the first output craft of the current source
    int cs = 0;
    for (long long i = 0; i < n_out; ++i) {
        long long s, c;
        if (craft_of) { s = source_of ? source_of[i] : 0; c = craft_of[i]; }
        else {
            while (i - first >= src[(size_t)cs].n) { first += src[(size_t)cs].n; ++cs; }
            s = cs; c = i - first;
        }
        const GatherSource<Seg> &g = src[(size_t)s];
        const bool dealt = g.slot && !g.slot->empty();
        plan.items[(size_t)s].push_back(GatherItem{i, c, dealt ? (long long)(*g.slot)[(size_t)c] : c});
        // the craft's slice of its source's CSR, rebased to where the output's CSR has got to
        const long long s0 = (*g.seg_off)[(size_t)c], s1 = (*g.seg_off)[(size_t)c + 1];
        plan.seg_off[(size_t)i] = (long long)plan.segs.size();
        plan.segs.insert(plan.segs.end(), g.segs->begin() + s0, g.segs->begin() + s1);
    }
    plan.seg_off[(size_t)n_out] = (long long)plan.segs.size();
    return plan;
}

}  // namespace eph
