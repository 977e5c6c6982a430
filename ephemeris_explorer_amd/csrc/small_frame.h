// small_frame.h -- the frame of the ONE-workgroup step kernels, stated once: k_lm_small (step_small.hip) and k_lm_double_small
// (step_double_small.hip) share the sizes, the zeroed LDS rows, the triangular pair decode, the pair phase, the ordered row sum,
// the step loop unrolled over the ring rotations and the ring write-back's slot arithmetic. What the (body, component) thread
// carries through the launch -- a plain state or a value and an error -- and everything that follows from it stays in each
// kernel's file. So do a dozen lines both kernels write out: the thread roles (chain, half, owner, owner_wave, my_i, cc, lvl, off,
// npairs, nrow) and the first load of sP. Moved into a function they change k_lm_small's code (the `?:` of my_i / cc become
// selects, a kernel-argument load is hoisted over the zeroing loop), and that kernel's code is held instruction for instruction
// (profiles/small_frame_refactor.md). For the same reason k_lm_small reaches small_decode and small_pair through local
// lambdas and has small_decode take its inputs by reference (its `In`).
// INCLUDED INSIDE namespace eph::pv<k>, behind pair_ns.h.
//
// Inside one workgroup the pair symmetry the reference uses CAN be shared: thread p owns the unordered pair
// (i, j), i < j, computes d, n2, 1/(n2*sqrt(n2)) once and writes both directed contributions
//     c(i<-j) =  d * (mu_j * inv)  -> U[i][j]   ("sources after the body")
//     c(j<-i) = -d * (mu_i * inv)  -> Lw[j][i]  ("sources before the body")
// exactly the reference's acceleration_paired halves. Rows of U / Lw are zero outside those ranges (written once
// at kernel start), so the two ordered chains of a body are plain in-order sums over a row (adding +0.0 is exact;
// the accumulators start at +0.0 and never become -0.0), one thread per (body, component, half):
//     ddy[i] = (0 + c(0,i) + ... + c(i-1,i)) + (0 + c(i,i+1) + ... + c(i,n-1)).
// Two barriers per step; history ring, velocity, predictor and Cowell formula live in the (body, component) thread.

constexpr int kSmallThreads = 512;        // eight waves: one unordered pair per thread (496 at 32 bodies), the 3 n chains x 2 halves in waves 0-2
constexpr int kSmallThreads2 = 256;       // the TWO form (gangs of more systems than CUs): four waves, two unordered pairs per thread
constexpr int kSmallMaxN = 32;           // bodies (the reference's shipped system has exactly 32); 33..64 -> k_lm_persistent
constexpr int kSmallRow = 32 + 2;        // doubles per row: 16-byte aligned rows an odd number of 16-byte units apart
constexpr int kSmallRows = 3 * kSmallMaxN;
static_assert(kSmallMaxN == kGangMaxN, "the launchers of dispatch.cpp admit what the kernels' rows hold");
using SmallRowsT = double[kSmallRows][kSmallRow];   // U / Lw: [body*3 + comp][source]

// the step loop unrolled over the L ring rotations: copy K runs at rotation (L - K) % L
// (ONE rolled copy of the step, the history shifted through the registers every step -- 24 v_mov_b64 -- instead of twelve copies,
// one per ring rotation (45 KB of code): measured slower at every gang size, profiles/r03_small_kernel_evidence.md.)
template <typename Step, int... Ks>
__device__ __forceinline__ void small_steps(Step &step, long long &s, long long nsteps, int &rot, bool &more,
                                            std::integer_sequence<int, Ks...>) {
    constexpr int L = sizeof...(Ks);
    (void)std::initializer_list<int>{(more ? (step(std::integral_constant<int, (L - Ks) % L>{}, s),
                                              rot = (L - Ks + L - 1) % L, more = ++s <= nsteps, 0)
                                           : 0)...};
}

// the rows start as zeros, and everything outside the chains' ranges stays zero
__device__ __forceinline__ void small_zero_rows(SmallRowsT &U, SmallRowsT &Lw, int tid) {
    for (int k = tid; k < kSmallRows * kSmallRow; k += blockDim.x) { (&U[0][0])[k] = 0.0; (&Lw[0][0])[k] = 0.0; }
}

// unordered pair q (i < j), row-major over the strict upper triangle (n <= 32: at most 496 pairs for 512 threads), decoded
// once. A slot without a pair runs pair (0, 1) again and stores nothing: straight-line code.
// (In: `int`, or `const int &` where the caller's code depends on it, see above)
template <typename In = int>
__device__ __forceinline__ void small_decode(In q, In n, In npairs, int &pi, int &pj) {
    pi = 0; pj = 1;
    if (q < npairs) {
        int i = 0;
        while ((i + 1) * (2 * n - i - 2) / 2 <= q) ++i;
        pi = i;
        pj = i + 1 + (q - i * (2 * n - i - 1) / 2);
    }
}

// The pair phase. Every thread runs the pair arithmetic: straight-line code, so the scheduler interleaves it with the predictor's
// position chain (sum1) instead of executing one exec-masked region after the other. The wrapper-free sqrt /
// reciprocal sequences run first and unconditionally; the range test that validates them (pair_term.h) is decided
// behind them, where the branch no longer stalls the wave, and an out-of-range operand anywhere in the wave redoes
// the term in the full IEEE form.
// `before_branch()` runs between the wrapper-free results and the (rare, wave-uniform) branch that redoes them in the full
// IEEE form: the owner waves pin the predictor's position chain there, so that it is emitted in the SAME block as the
// sequences and fills their issue gaps; without it the compiler places the chain behind the stores (round 5, read off the ISA).
// TWO: a second pair (wi, wj) -> (pi1, pj1) in the same thread; without it those arguments are dead.
template <bool TWO, typename Before>
__device__ __forceinline__ void small_pair(SmallRowsT &U, SmallRowsT &Lw, const double4 &vi, const double4 &vj, const double4 &wi,
                                           const double4 &wj, int pi0, int pj0, int pi1, int pj1, bool live0, bool live1,
                                           Before &&before_branch) {
    const double dx = vj.x - vi.x, dy = vj.y - vi.y, dz = vj.z - vi.z;
    const double n2 = dx * dx + dy * dy + dz * dz;
    double ex = 0.0, ey = 0.0, ez = 0.0, m2 = 1.0;
    if constexpr (TWO) { ex = wj.x - wi.x; ey = wj.y - wi.y; ez = wj.z - wi.z; m2 = ex * ex + ey * ey + ez * ez; }
    double ax, ay, az, bx, by, bz, cx = 0.0, cy = 0.0, cz = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    {
        // (TWO: the compiler emits the two reciprocal-cube sequences one after the other; writing them stage by stage with the
        // order pinned, as pair_finish_staged does for the workgroup kernel, was measured: no change, 0.87 us either way)
        const PairDen den = pair_den<true>(n2);
        pair_apply<true>(den, dx, dy, dz, vj.w, ax, ay, az);
        pair_apply<true>(den, -dx, -dy, -dz, vi.w, bx, by, bz);
        if constexpr (TWO) {
            const PairDen den1 = pair_den<true>(m2);
            pair_apply<true>(den1, ex, ey, ez, wj.w, cx, cy, cz);
            pair_apply<true>(den1, -ex, -ey, -ez, wi.w, gx, gy, gz);
        }
    }
    // the wrapper-free results exist HERE (otherwise the compiler sinks them into the else-side of the branch below)
    asm volatile("" : "+v"(ax), "+v"(ay), "+v"(az), "+v"(bx), "+v"(by), "+v"(bz));
    if constexpr (TWO) asm volatile("" : "+v"(cx), "+v"(cy), "+v"(cz), "+v"(gx), "+v"(gy), "+v"(gz));
    before_branch();
    if (__builtin_amdgcn_ballot_w64(!(in_range(n2) && (!TWO || in_range(m2)))) != 0) {
        const PairDen den = pair_den<false>(n2);
        pair_apply<false>(den, dx, dy, dz, vj.w, ax, ay, az);
        pair_apply<false>(den, -dx, -dy, -dz, vi.w, bx, by, bz);
        if constexpr (TWO) {
            const PairDen den1 = pair_den<false>(m2);
            pair_apply<false>(den1, ex, ey, ez, wj.w, cx, cy, cz);
            pair_apply<false>(den1, -ex, -ey, -ez, wi.w, gx, gy, gz);
        }
    }
    if (live0) {
        U[pi0 * 3 + 0][pj0] = ax;
        U[pi0 * 3 + 1][pj0] = ay;
        U[pi0 * 3 + 2][pj0] = az;
        Lw[pj0 * 3 + 0][pi0] = bx;
        Lw[pj0 * 3 + 1][pi0] = by;
        Lw[pj0 * 3 + 2][pi0] = bz;
    }
    if (live1) {
        U[pi1 * 3 + 0][pj1] = cx;
        U[pi1 * 3 + 1][pj1] = cy;
        U[pi1 * 3 + 2][pj1] = cz;
        Lw[pj1 * 3 + 0][pi1] = gx;
        Lw[pj1 * 3 + 1][pi1] = gy;
        Lw[pj1 * 3 + 2][pi1] = gz;
    }
}

// One ordered chain: the plain in-order sum over a row of `nrow` (16 or 32) doubles (zeros outside the chain's range; adding +0.0
// is exact and the sums never are -0.0), every read in flight before the first add. The partner half's sum sits in the adjacent
// lane: the kernels fetch it by a DPP quad permutation (dpp_xor1), not an LDS round trip (ds_bpermute).
template <int NB>
__device__ __forceinline__ double small_sum_blocks(const double *row) {
    double acc = 0.0;
    // (the optimiser hoists the common first eight reads and two adds of the two row lengths in front of the branch and
    // issues the long row's other eight reads behind sixteen adds. Forcing all sixteen reads in front of the first add
    // was SLOWER -- row sums 610 -> 677 ticks: a lone wave's ds_read_b128 costs it ~12 issue cycles each and overlaps
    // nothing of its own, profiles/r02_chain2_ubench.txt -- so the accident stays; round 5)
    double2 v[8 * NB];
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) v[k] = *reinterpret_cast<const double2 *>(row + 2 * k);
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) {
        acc = acc + v[k].x;
        acc = acc + v[k].y;
    }
    return acc;
}
__device__ __forceinline__ double small_row_sum(const double *row, int nrow) {
    if (nrow == 16) return small_sum_blocks<1>(row);
    return small_sum_blocks<2>(row);
}

// The ring write-back. After the launch register p of the owner thread holds level (newest - j), j = small_level(p, rot), where
// `rot` is the rotation small_steps left; that level's ring slot is (newest + j) % L.
template <int L>
__device__ __forceinline__ int small_newest_slot(int cur, long long nsteps) {     // slot of the newest level after nsteps
    return (int)(((long long)cur - nsteps % L + L) % L);
}
template <int L>
__device__ __forceinline__ int small_level(int p, int rot) { return (p - rot + L) % L; }
