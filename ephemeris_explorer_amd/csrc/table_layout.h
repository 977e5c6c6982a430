// table_layout.h -- the bookkeeping of the live device table (ephemeris_table.h) as a pure host value: which rows of the coefficient
// arrays each body owns and where its polynomials sit inside them. No device, no handle: the two operations below only do arithmetic
// and return a PLAN (the layout afterwards + the row ranges to upload), which the writer carries out and then stores. Plain C++
// (tests/table_layout_check.cpp compiles this header alone).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace eph {

// body b owns rows [base, base + cap); its polynomial i is row base + off + i, for i < npoly
struct BodyRegion {
    long long base = 0, cap = 0;
    long long off = 0;            // polynomial 0 inside the region
    long long npoly = 0;
    char grows_front = 0;         // the body has been prepended to: a fresh layout keeps headroom in front as well
    long long first_row() const { return base + off; }
};
// what a writer does to one body's spline, in polynomials
struct BodyUpdate {
    long long drop_front = 0, drop_back = 0;     // clear_before / clear_after
    long long add_front = 0, add_back = 0;       // prepend / append
};
// rows [row, row + count) receive polynomials [first, first + count) of body `body`, counted in its spline AS IT WILL BE after the update
struct RowUpload {
    int body = 0;
    long long row = 0, first = 0, count = 0;
};
struct TablePlan {
    bool fits = true;                  // false: lay the table out afresh (regions / uploads are empty then)
    std::vector<BodyRegion> regions;
    long long total = 0;               // rows of the whole table (a fresh layout only: following keeps the table's size)
    std::vector<RowUpload> uploads;
};

// Lay the table out afresh: every body's region gets room for as many polynomials again behind it (and in front, for a body that
// grows backwards), at least 32; regions are contiguous in body order. Every row is to be uploaded.
inline TablePlan lay_out_afresh(const std::vector<long long> &npoly, const std::vector<char> &grows_front) {
    TablePlan plan;
    const size_t nb = npoly.size();
    plan.regions.assign(nb, BodyRegion{});
    long long total = 0;
    for (size_t b = 0; b < nb; ++b) {
        const long long np = npoly[b];
        const long long room = std::max<long long>(np, 32);
        const long long front = grows_front[b] ? room : 0;
        BodyRegion &r = plan.regions[b];
        r.base = total;
        r.cap = front + np + room;
        r.off = front;
        r.npoly = np;
        r.grows_front = grows_front[b];
        total += r.cap;
        if (np) plan.uploads.push_back(RowUpload{(int)b, r.first_row(), 0, np});
    }
    plan.total = total;
    return plan;
}

// The spline counts and flags a fresh layout starts from once `up` has been applied to `regions`
inline void counts_after(const std::vector<BodyRegion> &regions, const std::vector<BodyUpdate> &up, std::vector<long long> *npoly,
                         std::vector<char> *grows_front) {
    npoly->assign(regions.size(), 0);
    grows_front->assign(regions.size(), 0);
    for (size_t b = 0; b < regions.size(); ++b) {
        (*npoly)[b] = regions[b].npoly - up[b].drop_front - up[b].drop_back + up[b].add_front + up[b].add_back;
        (*grows_front)[b] = regions[b].grows_front || up[b].add_front > 0;
    }
}

// Follow an update inside the regions as they are: a truncation moves two integers, an addition uploads the new rows only -- into
// headroom, never into a row that is published now (rows [first_row, first_row + npoly) of any body), so that a writer that fails half
// way has changed nothing a reader can see. A body whose new rows do not fit its region, or would land on rows it still publishes
// (dropped and added to on the same side in one update), makes the plan "does not fit".
inline TablePlan follow(const std::vector<BodyRegion> &regions, const std::vector<BodyUpdate> &up) {
    TablePlan plan;
    const size_t nb = regions.size();
    for (size_t b = 0; b < nb && plan.fits; ++b) {
        const BodyRegion &r = regions[b];
        const BodyUpdate &u = up[b];
        const long long off = r.off + u.drop_front;
        const long long np = r.npoly - u.drop_front - u.drop_back + u.add_front + u.add_back;     // the new count
        if (u.add_front > off || off - u.add_front + np > r.cap) plan.fits = false;
        if ((u.add_front && u.drop_front) || (u.add_back && u.drop_back)) plan.fits = false;
    }
    if (!plan.fits) return plan;
    plan.regions = regions;
    for (size_t b = 0; b < nb; ++b) {
        BodyRegion &r = plan.regions[b];
        const BodyUpdate &u = up[b];
        r.off += u.drop_front - u.add_front;
        r.npoly += u.add_front + u.add_back - u.drop_front - u.drop_back;
        if (u.add_front) r.grows_front = 1;
        if (u.add_front) plan.uploads.push_back(RowUpload{(int)b, r.first_row(), 0, u.add_front});
        if (u.add_back) plan.uploads.push_back(RowUpload{(int)b, r.first_row() + r.npoly - u.add_back, r.npoly - u.add_back, u.add_back});
    }
    return plan;
}

}  // namespace eph
