// table_layout_check.cpp -- a stand-alone model check of csrc/table_layout.h (built and run by tests/test_table_layout.py under
// AddressSanitizer and UBSan). Every body is a deque of polynomial ids, the device one vector of rows; seeded random appends,
// prepends, trims and merges are planned by the header, the plans' uploads executed into the rows, and after every operation the
// table is compared with the model by rules written here, not taken from the header's arithmetic.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <utility>
#include <vector>

#include "../ephemeris_explorer_amd/csrc/table_layout.h"

using namespace eph;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::fprintf(stderr, "%s:%d: op %ld: CHECK(%s) failed\n", __FILE__, __LINE__, g_op, #c); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)
static long g_op = 0;

int main() {
    std::mt19937_64 rng(20261018);
    auto upto = [&](long long hi) { return (long long)(rng() % (unsigned long long)(hi + 1)); };     // 0 .. hi
    long fits = 0, relayouts = 0;
    int next_id = 0;
    for (int nb = 1; nb <= 5; ++nb) {
        std::vector<std::deque<int>> model((size_t)nb);
        std::vector<char> grows_front((size_t)nb, 0);
        // the table as created: a fresh layout of the (random) first splines
        std::vector<long long> counts((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            counts[(size_t)b] = upto(100);
            for (long long k = 0; k < counts[(size_t)b]; ++k) model[(size_t)b].push_back(next_id++);
        }
        TablePlan plan = lay_out_afresh(counts, grows_front);
        std::vector<BodyRegion> regions;
        long long total = 0;
        std::vector<int> rows;
        bool fresh = true;
        std::vector<std::pair<long long, long long>> published;       // [first, last) per body before the operation (none at creation)
        for (long op = 0; op <= 25000; ++op, ++g_op) {
            std::vector<std::deque<int>> next = model;
            if (op > 0) {
                int kind = (int)upto(5);            // append, prepend, trim in front, trim behind, forward merge, backward merge
                for (const std::deque<int> &d : model)
                    if (d.size() > 300 && kind != 2 && kind != 3) kind = 2 + (int)upto(1);       // (long splines are trimmed: the walk stays small)
                std::vector<BodyUpdate> up((size_t)nb);
                for (int b = 0; b < nb; ++b) {
                    BodyUpdate &u = up[(size_t)b];
                    std::deque<int> &d = next[(size_t)b];
                    const long long size = (long long)d.size();
                    if (kind == 2 || kind == 5) u.drop_front = upto(std::min<long long>(100, size));
                    if (kind == 3 || kind == 4) u.drop_back = upto(std::min<long long>(100, size));
                    if (kind == 0 || kind == 4) u.add_back = upto(100);
                    if (kind == 1 || kind == 5) u.add_front = upto(100);
                    d.erase(d.begin(), d.begin() + u.drop_front);
                    d.erase(d.end() - u.drop_back, d.end());
                    std::vector<int> ids;
                    for (long long k = 0; k < u.add_front + u.add_back; ++k) ids.push_back(next_id++);
                    d.insert(d.begin(), ids.begin(), ids.begin() + u.add_front);
                    d.insert(d.end(), ids.begin() + u.add_front, ids.end());
                    if (u.add_front) grows_front[(size_t)b] = 1;
                    counts[(size_t)b] = (long long)d.size();
                }
                published.clear();
                for (const BodyRegion &r : regions) published.push_back({r.base + r.off, r.base + r.off + r.npoly});
                std::vector<long long> c2;
                std::vector<char> g2;
                counts_after(regions, up, &c2, &g2);
                CHECK(c2 == counts && g2 == grows_front);
                plan = follow(regions, up);
                fresh = !plan.fits;
                if (fresh) {
                    CHECK(plan.regions.empty() && plan.uploads.empty());
                    plan = lay_out_afresh(counts, grows_front);
                    ++relayouts;
                } else {
                    ++fits;
                }
            }
            if (fresh) {
                // the rule: room = max(np, 32), front = grows_front ? room : 0, cap = front + np + room, contiguous in body order
                long long at = 0;
                CHECK((int)plan.regions.size() == nb);
                for (int b = 0; b < nb; ++b) {
                    const BodyRegion &r = plan.regions[(size_t)b];
                    const long long np = counts[(size_t)b], room = np > 32 ? np : 32, front = grows_front[(size_t)b] ? room : 0;
                    CHECK(r.base == at && r.cap == front + np + room && r.off == front && r.npoly == np);
                    CHECK((r.grows_front != 0) == (grows_front[(size_t)b] != 0));
                    at += r.cap;
                }
                CHECK(plan.total == at);
                total = plan.total;
                rows.assign((size_t)total, -1);                        // fresh buffers: nothing of the old rows is published any more
                published.clear();
            }
            // carry the uploads out
            for (const RowUpload &u : plan.uploads) {
                CHECK(u.body >= 0 && u.body < nb && u.count > 0);
                const BodyRegion &r = plan.regions[(size_t)u.body];
                CHECK(u.row >= r.base && u.row + u.count <= r.base + r.cap);                     // inside the body's own region
                CHECK(u.first >= 0 && u.first + u.count <= (long long)next[(size_t)u.body].size());
                for (const auto &p : published) CHECK(u.row + u.count <= p.first || u.row >= p.second || p.first == p.second);
                for (long long k = 0; k < u.count; ++k) rows[(size_t)(u.row + k)] = next[(size_t)u.body][(size_t)(u.first + k)];
            }
            regions = plan.regions;
            model = next;
            // the table against the model
            long long end = 0;
            for (int b = 0; b < nb; ++b) {
                const BodyRegion &r = regions[(size_t)b];
                CHECK(r.cap >= 0 && r.base >= end);                                              // disjoint, in body order
                end = r.base + r.cap;
                CHECK(end <= total);                                                             // inside the total
                CHECK(r.off >= 0 && r.npoly >= 0 && r.off + r.npoly <= r.cap);                   // the polynomials inside the region
                CHECK(r.npoly == (long long)model[(size_t)b].size());
                for (long long i = 0; i < r.npoly; ++i) CHECK(rows[(size_t)(r.base + r.off + i)] == model[(size_t)b][(size_t)i]);
            }
        }
    }
    std::printf("operations %ld fits %ld relayouts %ld\n", g_op - 5, fits, relayouts);
    return 0;
}
