// mapf_env_large.hip -- MI355X (gfx950) kernels of the vectorised MAPF environment on maps of side 65..128.
//
// The kernels of mapf_env.hip hold a map row, an agent-occupancy row and a navigation-record word in one machine word (32 or 64
// bits).  Here a row is 128 bits: two uint64_t words (Row), with shifts carrying across the seam between column 63 and 64.  The
// rules are exactly those of mapf_env.hip (same step rules S0-S4, same parallel conflict-resolution fixed point -- the argument at
// the top of mapf_env.hip does not depend on the map size --, same navigation-record meaning, same scenario RNG keying); only the
// row type and the launch shapes differ.  Layouts: mapf_env_large.h.  One workgroup per environment, no packing, no tuning paths.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mapf_env.h"
#include "mapf_env_large.h"

namespace mapf_large {
namespace {

struct Row {
    uint64_t lo, hi;  // columns 0..63, 64..127
};
struct alignas(16) NaviRec {
    Row w[4];  // up, down, left, right
};
static_assert(sizeof(NaviRec) == 4 * kRowBytes, "a navigation record is 64 bytes");

__device__ __forceinline__ Row r_zero() { return Row{0ull, 0ull}; }
__device__ __forceinline__ Row r_or(Row a, Row b) { return Row{a.lo | b.lo, a.hi | b.hi}; }
__device__ __forceinline__ Row r_and(Row a, Row b) { return Row{a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ Row r_andn(Row a, Row b) { return Row{a.lo & ~b.lo, a.hi & ~b.hi}; }  // a & ~b
__device__ __forceinline__ bool r_any(Row a) { return (a.lo | a.hi) != 0ull; }
__device__ __forceinline__ int r_popc(Row a) { return __popcll(a.lo) + __popcll(a.hi); }
__device__ __forceinline__ Row r_bit(int y) { return y < 64 ? Row{1ull << y, 0ull} : Row{0ull, 1ull << (y - 64)}; }
__device__ __forceinline__ bool r_test(Row a, int y) { return ((y < 64 ? a.lo >> y : a.hi >> (y - 64)) & 1ull) != 0ull; }
// column y -> y + 1 (the bit of column 63 carries into the high word) and column y -> y - 1
__device__ __forceinline__ Row r_shl1(Row a) { return Row{a.lo << 1, (a.hi << 1) | (a.lo >> 63)}; }
__device__ __forceinline__ Row r_shr1(Row a) { return Row{(a.lo >> 1) | (a.hi << 63), a.hi >> 1}; }
// columns 0..L-1 (65 <= L <= 128)
__device__ __forceinline__ Row r_mask(int L) { return Row{~0ull, L >= 128 ? ~0ull : ((1ull << (L - 64)) - 1ull)}; }

// columns y-4 .. y+4 of a row -> bits 0..8 (columns outside the row read 0).  The one new bit trick: a window that starts at column
// 56..63 straddles the seam and takes its top bits from the high word.
__device__ __forceinline__ unsigned window9(Row a, int y) {
    const int s = y - 4;
    uint64_t v;
    if (s < 0) v = a.lo << (-s);
    else if (s >= 64) v = a.hi >> (s - 64);
    else if (s <= 55) v = a.lo >> s;
    else v = (a.lo >> s) | (a.hi << (64 - s));
    return (unsigned)v & 0x1FFu;
}

__device__ __forceinline__ Row shfl_row(Row a, int src) {
    const unsigned l0 = (unsigned)__shfl((int)(unsigned)a.lo, src, 64), l1 = (unsigned)__shfl((int)(unsigned)(a.lo >> 32), src, 64);
    const unsigned h0 = (unsigned)__shfl((int)(unsigned)a.hi, src, 64), h1 = (unsigned)__shfl((int)(unsigned)(a.hi >> 32), src, 64);
    return Row{((uint64_t)l1 << 32) | l0, ((uint64_t)h1 << 32) | h0};
}

// Map rows of one wavefront: lane i owns rows i (A) and i + 64 (B).  Chosen over a 128-lane workgroup with lane = row: the rows
// above and below a row are then reached by lane rotation alone (the seam rows 63 / 64 are lane 63's A and lane 0's B), with no LDS
// hand-off and no barrier per BFS level, and a wave-wide ballot ends the loop.  The frontier of row x - 1 (up) and x + 1 (down):
__device__ __forceinline__ void vert_neighbours(Row fa, Row fb, int lane, Row &upa, Row &upb, Row &dna, Row &dnb) {
    const int src_up = (lane + 63) & 63, src_dn = (lane + 1) & 63;
    const Row ra = shfl_row(fa, src_up), rb = shfl_row(fb, src_up);
    upa = lane ? ra : r_zero();  // row 0 has no row above
    upb = lane ? rb : ra;        // row 64's upper neighbour is row 63 = lane 63's A
    const Row da = shfl_row(fa, src_dn), db = shfl_row(fb, src_dn);
    dna = lane < 63 ? da : db;   // row 63's lower neighbour is row 64 = lane 0's B
    dnb = lane < 63 ? db : r_zero();
}

// ---------------------------------------------------------------------------------------------
// navi_kernel: Environment.get_navi_map (reference environment.py:217-276) as a bit-parallel BFS, one field per wavefront.  A cell
// first reached at level d from a frontier cell in direction k gets the reference's "neighbour k is strictly closer" flag.  The loop
// runs until the frontier is empty: at obstacle densities up to 0.5 a shortest path can be far longer than L.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) navi_kernel(int E, int E_handle, int L, int N, const Row *rows, const int16_t *goals, NaviRec *navi,
                                                   int32_t *status, const int32_t *env_ids, const uint8_t *env_mask) {
    const int lane = threadIdx.x & 63;
    const long long slot = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // (listed env, agent): one per wavefront
    if (slot >= (long long)E * N) return;  // (wave-uniform)
    int e = (int)(slot / N);
    if (env_ids) e = env_ids[e];
    if (e < 0 || e >= E_handle) return;  // (an id out of range is reported by the scatter kernel before this one)
    if (env_mask != nullptr && env_mask[e] == 0) return;
    const long long field = (long long)e * N + slot % N;
    const int xa = lane, xb = lane + 64;
    const bool inb = xb < L;
    const Row lm = r_mask(L);
    const Row freea = r_andn(lm, rows[(size_t)e * L + xa]);
    const Row freeb = inb ? r_andn(lm, rows[(size_t)e * L + xb]) : r_zero();
    int gx = goals[field * 2], gy = goals[field * 2 + 1];
    if (gx < 0 || gx >= L || gy < 0 || gy >= L) {
        if (lane == 0) atomicOr(status, kStatusRange);
        gx = -1;
        gy = 0;
    }
    Row visa = (xa == gx) ? r_bit(gy) : r_zero();  // dist[goal] = 0 unconditionally (:223)
    Row visb = (xb == gx) ? r_bit(gy) : r_zero();
    Row fa = visa, fb = visb;
    Row ua = r_zero(), ub = r_zero(), da = r_zero(), db = r_zero(), la = r_zero(), lb = r_zero(), ra = r_zero(), rb = r_zero();
    for (;;) {
        Row upa, upb, dna, dnb;
        vert_neighbours(fa, fb, lane, upa, upb, dna, dnb);
        const Row lfa = r_shl1(fa), lfb = r_shl1(fb), rfa = r_shr1(fa), rfb = r_shr1(fb);
        const Row na = r_andn(r_and(r_or(r_or(upa, dna), r_or(lfa, rfa)), freea), visa);
        const Row nb = r_andn(r_and(r_or(r_or(upb, dnb), r_or(lfb, rfb)), freeb), visb);
        ua = r_or(ua, r_and(na, upa));  // neighbour (x-1, y) strictly closer  (:260-262)
        ub = r_or(ub, r_and(nb, upb));
        da = r_or(da, r_and(na, dna));  // (x+1, y)                           (:264-266)
        db = r_or(db, r_and(nb, dnb));
        la = r_or(la, r_and(na, lfa));  // (x, y-1)                           (:268-270)
        lb = r_or(lb, r_and(nb, lfb));
        ra = r_or(ra, r_and(na, rfa));  // (x, y+1)                           (:272-274)
        rb = r_or(rb, r_and(nb, rfb));
        visa = r_or(visa, na);
        visb = r_or(visb, nb);
        fa = na;
        fb = nb;
        if (__ballot(r_any(na) || r_any(nb)) == 0ull) break;
    }
    NaviRec rec;
    rec.w[0] = ua, rec.w[1] = da, rec.w[2] = la, rec.w[3] = ra;
    navi[field * L + xa] = rec;
    if (inb) {
        rec.w[0] = ub, rec.w[1] = db, rec.w[2] = lb, rec.w[3] = rb;
        navi[field * L + xb] = rec;
    }
}

// ---------------------------------------------------------------------------------------------
// step_kernel: Environment.step + observe (reference environment.py:278-467) for one environment per workgroup, one lane per agent
// (NT >= N).  The step phase is mapf_env_step_body.inc's for one environment: occupant lookup through a padded id grid in LDS, rule
// (b) from the 4 neighbours of the target cell, rule (a) iterated to its fixed point.  The observation is assembled as a bit string
// in LDS (bit b = output byte b of the environment's block) by (agent, window row) tasks and expanded to bytes.
// actions == nullptr: observe only (mapf_observe / mapf_observe_masked).
// ---------------------------------------------------------------------------------------------
constexpr int R = 4, WW = 2 * R + 1;
constexpr int kMaxGrid = (kMaxLen + 2) * (kMaxLen + 2);

__device__ __forceinline__ void deposit_field(unsigned *bits, unsigned off, unsigned v) {
    if (v) {
        const unsigned d = off >> 5, sh = off & 31u;
        atomicOr(&bits[d], v << sh);
        if (sh > 32u - WW) atomicOr(&bits[d + 1], v >> (32u - sh));
    }
}
__device__ __forceinline__ unsigned expand4m(unsigned nib) { return __umul24(nib, 0x00204081u) & 0x01010101u; }

template <int NT>
__global__ void __launch_bounds__(NT) step_kernel(StepArgs p) {
    const int e = blockIdx.x, t = threadIdx.x;
    const bool do_step = p.actions != nullptr;
    const bool do_obs = p.obs != nullptr || p.obs_bits != nullptr;
    if (!do_step && p.mask != nullptr && p.mask[e] == 0) return;  // masked observe: this environment's outputs stay as they are
    const int L = p.L, N = p.N;
    const int LP = L + 2 * R, GP = L + 2;
    const int grid_q = (GP * GP + 15) >> 4;
    const int bits_q = ((N * 6 * WW * WW + 31) / 32 + 1 + 3) >> 2;
    __shared__ Row s_obst[kMaxLen + 2 * R], s_agent[kMaxLen + 2 * R];  // map row x at index x + R; the border rows read 0
    __shared__ uint4 s_id4[(kMaxGrid + 15) / 16];                       // agent id per cell (1-cell border), 0xFF = empty
    extern __shared__ uint4 s_bits4[];  // [bits_q] (dynamic: sized by the agent count, step_smem_bytes)
    __shared__ unsigned short s_next[NT], s_cur[NT];
    __shared__ unsigned char s_mov[NT];
    unsigned char *s_id = reinterpret_cast<unsigned char *>(s_id4);
    unsigned *s_bits = reinterpret_cast<unsigned *>(s_bits4);

    const bool agent = t < N;
    const size_t own = (size_t)e * N + (agent ? t : 0);
    const short2 cpos = *reinterpret_cast<const short2 *>(p.agents + own * 2);
    short2 gpos = make_short2(0, 0);
    int act = 0;
    if (do_step) {
        gpos = *reinterpret_cast<const short2 *>(p.goals + own * 2);
        act = p.actions[own];
    }
    const Row *map_rows = reinterpret_cast<const Row *>(p.map_rows) + (size_t)e * L;
    for (int r = t; r < LP; r += NT) {
        const int rr = r - R;
        s_obst[r] = (rr >= 0 && rr < L) ? map_rows[rr] : r_zero();
        s_agent[r] = r_zero();
    }
    if (do_step)
        for (int k = t; k < grid_q; k += NT) s_id4[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (do_obs)
        for (int k = t; k < bits_q; k += NT) s_bits4[k] = make_uint4(0u, 0u, 0u, 0u);
    // a position outside the map (only after a load / mapf_set_agents that raised kStatusRange) is clamped: every LDS index below
    // (id grid, occupancy rows, window rows) then stays inside its table
    const int cx = min(max((int)cpos.x, 0), L - 1), cy = min(max((int)cpos.y, 0), L - 1), gx = gpos.x, gy = gpos.y;
    int nx = cx, ny = cy;
    int rc = MAPF_RC_STAY_ON_GOAL;
    int all_done = 0;
    __syncthreads();

    if (do_step) {
        bool mover = false;
        if (agent) {
            if (act < 0 || act > 4) {  // reference: AssertionError (environment.py:290)
                atomicOr(p.status, kStatusAction);
                act = 0;
            }
            // S0 (environment.py:298-311)
            mover = act != 0;
            nx = cx + (act == 2) - (act == 1);  // action_list, environment.py:12
            ny = cy + (act == 4) - (act == 3);
            rc = mover ? MAPF_RC_MOVE : ((cx == gx && cy == gy) ? MAPF_RC_STAY_ON_GOAL : MAPF_RC_STAY_OFF_GOAL);
            // S1 (environment.py:320-332; :322 tests both coordinates against map_size[0] -- the maps are square)
            if (mover) {
                bool blocked = nx < 0 || ny < 0 || nx >= L || ny >= L;
                if (!blocked) blocked = r_test(s_obst[nx + R], ny);
                if (blocked) {
                    mover = false;
                    rc = MAPF_RC_COLLISION;
                    nx = cx;
                    ny = cy;
                }
            }
            s_id[(cx + 1) * GP + cy + 1] = (unsigned char)t;
            s_next[t] = (unsigned short)((nx << 8) | ny);
            s_mov[t] = mover;
        }
        __syncthreads();

        // S2 swap (environment.py:335-365)
        const unsigned my_cur = (unsigned)((cx << 8) | cy);
        const unsigned my_next = (unsigned)((nx << 8) | ny);
        int occ = 0xFF;
        bool swap = false;
        if (mover) {
            occ = s_id[(nx + 1) * GP + ny + 1];
            if (occ != 0xFF) swap = s_mov[occ] && s_next[occ] == my_cur;
        }
        __syncthreads();
        if (swap) {
            mover = false;
            rc = MAPF_RC_COLLISION;
            nx = cx;
            ny = cy;
            s_next[t] = (unsigned short)my_cur;
            s_mov[t] = 0;
        }
        __syncthreads();

        // S3 vertex (environment.py:368-406), rule (b): a lower-id mover claims the same cell (rivals stand on its 4 neighbours)
        bool lose = false;
        if (mover) {
            const int c = (nx + 1) * GP + ny + 1;
            const int nb[4] = {c - GP, c + GP, c - 1, c + 1};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = s_id[nb[q]];
                if (j < t) lose |= (s_mov[j] && s_next[j] == my_next);
            }
        }
        // rule (a) + cascade: target cell held by an agent that is (now) settled
        for (int round = 0; round <= N; ++round) {
            const bool revert = mover && (lose || (occ != 0xFF && !s_mov[occ]));
            const int any = __syncthreads_or(revert);
            if (revert) {
                mover = false;
                rc = MAPF_RC_COLLISION;
                nx = cx;
                ny = cy;
                s_mov[t] = 0;
            }
            if (!any) break;
            __syncthreads();
        }

        // S4 (environment.py:410-430)
        all_done = __syncthreads_and(!agent || (nx == gx && ny == gy));
        if (all_done) rc = MAPF_RC_FINISH;
    }

    // ---- agent occupancy rows after the step (+ the overlap invariant, environment.py:424-428) ----
    if (agent) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(ny < 64 ? &s_agent[nx + R].lo : &s_agent[nx + R].hi);
        const unsigned long long bit = 1ull << (ny & 63);
        const unsigned long long old = atomicOr(w, bit);
        if (do_step && (old & bit)) atomicOr(p.status, kStatusOverlap);
        s_cur[t] = (unsigned short)((nx << 8) | ny);
    }
    if (do_obs) {
        __syncthreads();
        // ---- one task per (agent, window row): 6 channel fields of 9 bits ----
        const NaviRec *navi = reinterpret_cast<const NaviRec *>(p.navi) + (size_t)e * N * L;
        for (int q = t; q < N * WW; q += NT) {
            const int i = q / WW, dy = q - i * WW;
            const unsigned key = s_cur[i];
            const int x = key >> 8, y = key & 255;
            const int row = x - R + dy;  // LDS index row + R = x + dy; rows outside the map read 0 ("out of bounds reads as free")
            unsigned f_ag = window9(s_agent[x + dy], y);
            if (dy == R) f_ag &= ~(1u << R);  // centre of channel 0 forced to 0 (environment.py:461)
            const unsigned f_ob = window9(s_obst[x + dy], y);
            const unsigned off = (unsigned)((i * 6 * WW + dy) * WW);
            deposit_field(s_bits, off, f_ag);
            deposit_field(s_bits, off + WW * WW, f_ob);
            if (row >= 0 && row < L) {
                const NaviRec rec = navi[(size_t)i * L + row];
#pragma unroll
                for (int k = 0; k < 4; ++k) deposit_field(s_bits, off + (2 + k) * WW * WW, window9(rec.w[k], y));
            }
        }
        __syncthreads();

        const int total = N * 6 * WW * WW;
        if (p.obs_bits) {  // bit-packed observation row (the replay's storage format)
            uint32_t *ob = p.obs_bits + (size_t)e * p.obs_bits_rd;
            const int nd = (total + 31) >> 5;
            for (int k = t; k < p.obs_bits_rd; k += NT) ob[k] = k < nd ? s_bits[k] : 0u;
        }
        if (p.obs) {  // expand the bit string: bit b -> byte b of this environment's observation block
            uint8_t *out = p.obs + (size_t)e * total;
            const uintptr_t a = reinterpret_cast<uintptr_t>(p.obs);
            if (total % 16 == 0 && (a & 15) == 0) {
                const unsigned short *b16 = reinterpret_cast<const unsigned short *>(s_bits);
                for (int task = t; task < (total >> 4); task += NT) {
                    const unsigned bits = b16[task];
                    reinterpret_cast<uint4 *>(out)[task] =
                        make_uint4(expand4m(bits & 15u), expand4m((bits >> 4) & 15u), expand4m((bits >> 8) & 15u), expand4m(bits >> 12));
                }
            } else if (total % 4 == 0 && (a & 3) == 0) {
                for (int task = t; task < (total >> 2); task += NT)
                    reinterpret_cast<unsigned *>(out)[task] = expand4m((s_bits[task >> 3] >> ((task & 7) * 4)) & 15u);
            } else {
                for (int b = t; b < total; b += NT) out[b] = (uint8_t)((s_bits[b >> 5] >> (b & 31)) & 1u);
            }
        }
    }

    // ---- small result stores ----
    if (agent) {
        const size_t o = (size_t)e * N + t;
        if (do_step) {
            *reinterpret_cast<short2 *>(p.agents + o * 2) = make_short2((short)nx, (short)ny);
            if (p.rclass) p.rclass[o] = (int8_t)rc;
            if (p.reward) p.reward[o] = p.rtab[rc];
        }
        if (p.pos_out) *reinterpret_cast<short2 *>(p.pos_out + o * 2) = make_short2((short)nx, (short)ny);
    }
    if (do_step && t == 0) {
        if (p.done) p.done[e] = (uint8_t)(all_done != 0);
        p.steps[e] += 1;
    }
}

// ---------------------------------------------------------------------------------------------
// reset_kernel: on-device scenario generation for the environments flagged in `mask` (Environment.reset, reference
// environment.py:146-196 / __init__ :100-143), the rule and the counter-based RNG keying of mapf_env.hip's reset_body (placement
// only; the navigation fields are built by navi_kernel behind it).  One wavefront per environment, lane i = rows i and i + 64.
//   map        Bernoulli(rho) per cell, rho = density or ~ triangular(0, 0.33, 0.5)
//   placement  the goal uniform over the remaining cells of partitions (components found by flood fill) that still hold >= 2 of
//              them, the start uniform over the rest of the goal's partition == the reference's partition weighted by its size
//   a map that cannot host N agents is re-drawn.
// STAGE (mapf_stage_next): the scenario of epoch + 1 is drawn into the staging arrays, st_need[e] tells navi_kernel whether the
// environment was re-drawn; the live epoch and step counters are not touched.  Same draws as the direct reset of that epoch.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ float u01(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}
// position of the k-th (0-based) set bit of a word
__device__ __forceinline__ int nth_bit(uint64_t w, int k) {
    for (; k > 0; --k) w &= w - 1;
    return (int)__ffsll((unsigned long long)w) - 1;
}
// column of the k-th set bit of a row
__device__ __forceinline__ int nth_bit(Row a, int k) {
    const int pl = __popcll(a.lo);
    return k < pl ? nth_bit(a.lo, k) : 64 + nth_bit(a.hi, k - pl);
}

// wave-wide: the r-th (0-based) set bit of the rows (A of every lane, then B of every lane: row order) -> (x, y) on every lane
__device__ __forceinline__ void select_bit(Row a, Row b, int r, int lane, int &x, int &y) {
    const int ca = r_popc(a), cb = r_popc(b);
    const int ia = wave_incl_scan(ca, lane), ib = wave_incl_scan(cb, lane);
    const int tot_a = __shfl(ia, 63, 64);
    const int ea = ia - ca, eb = tot_a + ib - cb;
    const bool mine_a = r >= ea && r < ia, mine_b = r >= eb && r < eb + cb;
    int yy = 0;
    if (mine_a) yy = nth_bit(a, r - ea);
    else if (mine_b) yy = nth_bit(b, r - eb);
    const unsigned long long wa = __ballot(mine_a), wb = __ballot(mine_b);
    const int src = wa ? (int)__ffsll(wa) - 1 : (wb ? (int)__ffsll(wb) - 1 : 0);
    x = wa ? src : src + 64;
    y = __shfl(yy, src, 64);
}

constexpr int kCachedParts = 8;  // partitions of the current map kept in LDS (8 x 2 KiB)

template <bool STAGE>
__global__ void __launch_bounds__(64) reset_kernel(int E, int L, int N, const uint8_t *mask, float density, uint64_t seed, Row *map_rows,
                                                   int16_t *agents, int16_t *goals, int32_t *steps, int32_t *epochs, int32_t *status,
                                                   int32_t *st_epoch, uint8_t *st_need) {
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= E || (mask && !mask[e])) return;
    __shared__ Row s_part[kCachedParts][kMaxLen];  // row sets of the partitions seen on the current map
    const int xa = lane, xb = lane + 64;
    const bool inb = xb < L;
    const Row lm = r_mask(L);
    int epoch = 0;
    if (STAGE) {
        epoch = epochs[e] + 1;
        const bool have = st_epoch[e] == epoch;
        if (lane == 0) st_need[e] = have ? 0 : 1;
        if (have) return;
    } else {
        if (lane == 0) epoch = atomicAdd(&epochs[e], 1) + 1;
        epoch = __shfl(epoch, 0, 64);
    }
    const uint64_t base = mix64(seed ^ mix64(((uint64_t)e << 32) | (uint32_t)epoch));
    bool ok = false;
    Row oa = r_zero(), ob = r_zero();
    for (int attempt = 0; attempt < 64 && !ok; ++attempt) {
        const uint64_t akey = mix64(base + (uint64_t)attempt);
        float rho = density;
        if (density < 0.f) {  // np.random.triangular(0, 0.33, 0.5)
            const float u = u01(mix64(akey ^ 0x7269616E67ull));
            const float a = 0.f, c = 0.33f, b = 0.5f;
            rho = (u < (c - a) / (b - a)) ? a + sqrtf(u * (b - a) * (c - a)) : b - sqrtf((1.f - u) * (b - a) * (b - c));
        }
        oa = ob = r_zero();
        for (int y = 0; y < L; ++y) {
            if (u01(mix64(akey + 0x100 + (uint64_t)(xa * L + y))) < rho) oa = r_or(oa, r_bit(y));
            if (inb && u01(mix64(akey + 0x100 + (uint64_t)(xb * L + y))) < rho) ob = r_or(ob, r_bit(y));
        }
        const Row freea = r_andn(lm, oa), freeb = inb ? r_andn(lm, ob) : r_zero();
        Row avail_a = freea, avail_b = freeb, elig_a = freea, elig_b = freeb;
        ok = true;
        int nparts = 0;  // (wave-uniform)
        uint64_t draw = akey ^ 0x64726177ull;
        for (int i = 0; i < N && ok; ++i) {
            int gx = 0, gy = 0, cnt = 0;
            Row vis_a = r_zero(), vis_b = r_zero();
            for (;;) {  // rejection over candidate goal cells; every rejection removes >= 1 candidate
                const int total = wave_sum(r_popc(elig_a) + r_popc(elig_b));
                if (total == 0) {
                    ok = false;
                    break;
                }
                draw = mix64(draw);
                select_bit(elig_a, elig_b, (int)(draw % (uint64_t)total), lane, gx, gy);
                int hit = -1;
                for (int k = 0; k < nparts && hit < 0; ++k)
                    if (r_test(s_part[k][gx], gy)) hit = k;  // (one address for the whole wave)
                if (hit >= 0) {
                    vis_a = s_part[hit][xa];
                    vis_b = s_part[hit][xb];
                } else {  // flood fill of the goal's partition
                    vis_a = (xa == gx) ? r_bit(gy) : r_zero();
                    vis_b = (xb == gx) ? r_bit(gy) : r_zero();
                    Row fa = vis_a, fb = vis_b;
                    for (;;) {
                        Row upa, upb, dna, dnb;
                        vert_neighbours(fa, fb, lane, upa, upb, dna, dnb);
                        const Row na = r_andn(r_and(r_or(r_or(upa, dna), r_or(r_shl1(fa), r_shr1(fa))), freea), vis_a);
                        const Row nb = r_andn(r_and(r_or(r_or(upb, dnb), r_or(r_shl1(fb), r_shr1(fb))), freeb), vis_b);
                        vis_a = r_or(vis_a, na);
                        vis_b = r_or(vis_b, nb);
                        fa = na;
                        fb = nb;
                        if (__ballot(r_any(na) || r_any(nb)) == 0ull) break;
                    }
                    if (nparts < kCachedParts) {
                        s_part[nparts][xa] = vis_a;
                        s_part[nparts][xb] = vis_b;
                        ++nparts;
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                cnt = wave_sum(r_popc(r_and(vis_a, avail_a)) + r_popc(r_and(vis_b, avail_b)));
                if (cnt >= 2) break;
                elig_a = r_andn(elig_a, vis_a);  // this partition holds < 2 remaining cells: never a candidate again
                elig_b = r_andn(elig_b, vis_b);
            }
            if (!ok) break;
            const Row ga = (xa == gx) ? r_bit(gy) : r_zero(), gb = (xb == gx) ? r_bit(gy) : r_zero();
            avail_a = r_andn(avail_a, ga), avail_b = r_andn(avail_b, gb);
            elig_a = r_andn(elig_a, ga), elig_b = r_andn(elig_b, gb);
            int sx, sy;
            draw = mix64(draw);
            select_bit(r_and(vis_a, avail_a), r_and(vis_b, avail_b), (int)(draw % (uint64_t)(cnt - 1)), lane, sx, sy);
            const Row sa = (xa == sx) ? r_bit(sy) : r_zero(), sb = (xb == sx) ? r_bit(sy) : r_zero();
            avail_a = r_andn(avail_a, sa), avail_b = r_andn(avail_b, sb);
            elig_a = r_andn(elig_a, sa), elig_b = r_andn(elig_b, sb);
            if (cnt - 2 < 2) elig_a = r_andn(elig_a, vis_a), elig_b = r_andn(elig_b, vis_b);
            const size_t o = (size_t)e * N + i;
            if (lane == 0) {
                goals[o * 2] = (int16_t)gx;
                goals[o * 2 + 1] = (int16_t)gy;
                agents[o * 2] = (int16_t)sx;
                agents[o * 2 + 1] = (int16_t)sy;
            }
        }
    }
    if (ok) {
        map_rows[(size_t)e * L + xa] = oa;
        if (inb) map_rows[(size_t)e * L + xb] = ob;
    }
    if (lane == 0) {
        if (STAGE) {
            if (ok) st_epoch[e] = epoch;
            else st_need[e] = 0, atomicOr(status, kStatusRange);
        } else {
            if (ok) steps[e] = 0;
            else atomicOr(status, kStatusRange);
        }
    }
}

// mapf_reset_envs with a staged scenario: map rows, positions, goals and navigation records of the flagged environments are
// copied over (16-byte chunks) and the epoch advances.  Nothing staged for the next epoch raises kStatusStage.
__global__ void __launch_bounds__(256) stage_swap_kernel(int E, int L, int N, const uint8_t *mask, Row *map_rows, int16_t *agents, int16_t *goals,
                                                         NaviRec *navi, int32_t *steps, int32_t *epochs, int32_t *status, const Row *st_map_rows,
                                                         const int16_t *st_agents, const int16_t *st_goals, const NaviRec *st_navi,
                                                         const int32_t *st_epoch) {
    const int e = blockIdx.x, tid = threadIdx.x;
    if (e >= E || (mask && !mask[e])) return;
    const int epoch = epochs[e] + 1;
    if (st_epoch[e] != epoch) {
        if (tid == 0) atomicOr(status, kStatusStage);
        return;
    }
    const size_t nchunk = (size_t)N * L * sizeof(NaviRec) / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(st_navi + (size_t)e * N * L);
    uint4 *dst = reinterpret_cast<uint4 *>(navi + (size_t)e * N * L);
    for (size_t i = tid; i < nchunk; i += 256) dst[i] = src[i];
    for (int i = tid; i < L; i += 256) map_rows[(size_t)e * L + i] = st_map_rows[(size_t)e * L + i];
    for (int i = tid; i < 2 * N; i += 256) {
        agents[(size_t)e * N * 2 + i] = st_agents[(size_t)e * N * 2 + i];
        goals[(size_t)e * N * 2 + i] = st_goals[(size_t)e * N * 2 + i];
    }
    __syncthreads();  // (every thread has read epochs[e])
    if (tid == 0) {
        epochs[e] = epoch;
        steps[e] = 0;
    }
}

// ---- loads and read-back ----
__global__ void pack_map_kernel(int E, int L, const int8_t *maps, Row *rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)E * L) return;
    const int8_t *m = maps + idx * L;
    Row w = r_zero();
    for (int y = 0; y < L; ++y)
        if (m[y] != 0) w = r_or(w, r_bit(y));
    rows[idx] = w;
}

__global__ void unpack_map_kernel(int E, int L, const Row *rows, int8_t *maps) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)E * L * L) return;
    const long long r = idx / L;
    maps[idx] = (int8_t)r_test(rows[r], (int)(idx - r * L));
}

__global__ void scatter_load_kernel(int n, int L, int N, const int32_t *ids, const int8_t *maps, const int16_t *agents, const int16_t *goals,
                                    Row *rows, int16_t *dst_agents, int16_t *dst_goals, int32_t *steps, int E, int32_t *status) {
    const int k = blockIdx.x;
    const int e = ids[k];
    if (e < 0 || e >= E) {
        if (threadIdx.x == 0) atomicOr(status, kStatusRange);
        return;
    }
    for (int r = threadIdx.x; r < L; r += blockDim.x) {
        const int8_t *m = maps + ((size_t)k * L + r) * L;
        Row w = r_zero();
        for (int y = 0; y < L; ++y)
            if (m[y] != 0) w = r_or(w, r_bit(y));
        rows[(size_t)e * L + r] = w;
    }
    for (int q = threadIdx.x; q < N * 2; q += blockDim.x) {
        const int16_t a = agents[(size_t)k * N * 2 + q], g = goals[(size_t)k * N * 2 + q];
        if (a < 0 || a >= L || g < 0 || g >= L) atomicOr(status, kStatusRange);
        dst_agents[(size_t)e * N * 2 + q] = a;
        dst_goals[(size_t)e * N * 2 + q] = g;
    }
    if (threadIdx.x == 0) steps[e] = 0;
}

// navigation records -> uint8 [E][N][4][L][L]
__global__ void unpack_navi_kernel(long long fields, int L, const NaviRec *navi, uint8_t *out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= fields * 4 * L * L) return;
    const int y = (int)(idx % L);
    long long q = idx / L;
    const int x = (int)(q % L);
    q /= L;
    const int k = (int)(q % 4);
    out[idx] = (uint8_t)r_test(navi[(q / 4) * L + x].w[k], y);
}

inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

hipError_t step(const StepArgs &a, hipStream_t s) {
    // one workgroup per environment, one lane per agent: a single wavefront up to 64 agents, four above.  Dynamic LDS: the
    // observation bit string (+1 spill dword, whole uint4s)
    const size_t smem = (size_t)(((a.N * 6 * WW * WW + 31) / 32 + 1 + 3) >> 2) * 16;
    if (a.N <= 64) hipLaunchKernelGGL(step_kernel<64>, dim3(a.E), dim3(64), smem, s, a);
    else hipLaunchKernelGGL(step_kernel<256>, dim3(a.E), dim3(256), smem, s, a);
    return hipGetLastError();
}

hipError_t pack_maps(int E, int L, const int8_t *maps, void *rows, hipStream_t s) {
    hipLaunchKernelGGL(pack_map_kernel, dim3(blocks_for((long long)E * L, 256)), dim3(256), 0, s, E, L, maps, static_cast<Row *>(rows));
    return hipGetLastError();
}

hipError_t unpack_maps(int E, int L, const void *rows, int8_t *maps, hipStream_t s) {
    hipLaunchKernelGGL(unpack_map_kernel, dim3(blocks_for((long long)E * L * L, 256)), dim3(256), 0, s, E, L, static_cast<const Row *>(rows), maps);
    return hipGetLastError();
}

hipError_t scatter_load(int n, int L, int N, const int32_t *ids, const int8_t *maps, const int16_t *agents, const int16_t *goals, void *rows,
                        int16_t *dst_agents, int16_t *dst_goals, int32_t *steps, int E, int32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(scatter_load_kernel, dim3(n), dim3(128), 0, s, n, L, N, ids, maps, agents, goals, static_cast<Row *>(rows), dst_agents,
                       dst_goals, steps, E, status);
    return hipGetLastError();
}

hipError_t build_navi(int E, int E_handle, int L, int N, const void *rows, const int16_t *goals, void *navi, int32_t *status, const int32_t *env_ids,
                      const uint8_t *env_mask, hipStream_t s) {
    const long long fields = (long long)E * N;  // one wavefront each, four per workgroup
    hipLaunchKernelGGL(navi_kernel, dim3(blocks_for(fields * 64, 256)), dim3(256), 0, s, E, E_handle, L, N, static_cast<const Row *>(rows), goals,
                       static_cast<NaviRec *>(navi), status, env_ids, env_mask);
    return hipGetLastError();
}

hipError_t unpack_navi(long long fields, int L, const void *navi, uint8_t *out, hipStream_t s) {
    hipLaunchKernelGGL(unpack_navi_kernel, dim3(blocks_for(fields * 4 * L * L, 256)), dim3(256), 0, s, fields, L, static_cast<const NaviRec *>(navi),
                       out);
    return hipGetLastError();
}

hipError_t reset(int E, int L, int N, const uint8_t *mask, float density, uint64_t seed, void *rows, int16_t *agents, int16_t *goals, void *navi,
                 int32_t *steps, int32_t *epochs, int32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(reset_kernel<false>, dim3(E), dim3(64), 0, s, E, L, N, mask, density, seed, static_cast<Row *>(rows), agents, goals, steps,
                       epochs, status, (int32_t *)nullptr, (uint8_t *)nullptr);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return build_navi(E, E, L, N, rows, goals, navi, status, nullptr, mask, s);
}

hipError_t stage_fill(int E, int L, int N, float density, uint64_t seed, void *st_rows, int16_t *st_agents, int16_t *st_goals, void *st_navi,
                      const int32_t *epochs, int32_t *status, int32_t *st_epoch, uint8_t *st_need, hipStream_t s) {
    hipLaunchKernelGGL(reset_kernel<true>, dim3(E), dim3(64), 0, s, E, L, N, (const uint8_t *)nullptr, density, seed, static_cast<Row *>(st_rows),
                       st_agents, st_goals, (int32_t *)nullptr, const_cast<int32_t *>(epochs), status, st_epoch, st_need);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return build_navi(E, E, L, N, st_rows, st_goals, st_navi, status, nullptr, st_need, s);
}

hipError_t stage_swap(int E, int L, int N, const uint8_t *mask, void *rows, int16_t *agents, int16_t *goals, void *navi, int32_t *steps,
                      int32_t *epochs, int32_t *status, const void *st_rows, const int16_t *st_agents, const int16_t *st_goals,
                      const void *st_navi, const int32_t *st_epoch, hipStream_t s) {
    hipLaunchKernelGGL(stage_swap_kernel, dim3(E), dim3(256), 0, s, E, L, N, mask, static_cast<Row *>(rows), agents, goals,
                       static_cast<NaviRec *>(navi), steps, epochs, status, static_cast<const Row *>(st_rows), st_agents, st_goals,
                       static_cast<const NaviRec *>(st_navi), st_epoch);
    return hipGetLastError();
}

}  // namespace mapf_large
