// Row step of the deterministic search (search="beam"): per (image, beam) row the `beam` most likely tokens and their model
// log-probabilities -- no noise, no top-k filter, no re-normalisation over the picks.
//   pass 1 : ONE sweep over the row (16-byte loads) with an online (max, sum) of x * (1 / T) per lane -> lse = logsumexp(x / T) over every
//            real column; the same sweep leaves every thread the best eligible column it saw (eligible: not unk, > -inf).
//   bound  : the beam-th largest of the 256 thread bests is a column of the row, and `beam` distinct columns reach it, so it is a lower
//            bound of the beam-th largest eligible logit; on real logits a handful of columns more than `beam` reach it.
//   pass 2 : every eligible column that reaches the bound goes to an LDS buffer (the row is L2-resident by now; with group maxima only
//            the 64-column groups whose maximum reaches the bound are read), and the `beam` best of the buffer are ranked there.
//   flat   : more columns at the bound than the buffer holds: `beam` rounds of block arg-max over the row instead.
// Order: a column is the 64-bit key (order-preserving key of x, ~index): larger logit first, equal logits to the lower index; -0.0 and
// +0.0 compare equal.  Keys are unique, every reduction is an integer maximum or a float sum in a fixed tree: two runs are bit-identical.
#include "common.h"
#include "prof.h"

#define BEST_CAP DH_BEAM_MAX_SURVIVORS
#define BEST_NT 256

typedef unsigned long long best_key_t;

// larger float <=> larger key; -0.0 and +0.0 share one key (beam.hip's f2key)
__device__ __forceinline__ uint32_t best_f2key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// 0 for a column that can never be picked (unk, -inf, NaN); every other key is > 0 and names its column
__device__ __forceinline__ best_key_t best_key(float x, int c, int unk) {
    return (c != unk && x > -INFINITY) ? ((best_key_t)best_f2key(x) << 32) | (best_key_t)(0xFFFFFFFFu - (uint32_t)c) : 0ull;
}
__device__ __forceinline__ int best_key_col(best_key_t k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// maximum over the block, the same value in every thread (LDS tree; red: BEST_NT keys)
__device__ __forceinline__ best_key_t best_block_max(best_key_t v, best_key_t* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = BEST_NT / 2; s > 0; s >>= 1) {
        if (tid < s) { const best_key_t o = red[tid + s]; if (o > red[tid]) red[tid] = o; }
        __syncthreads();
    }
    const best_key_t r = red[0];
    __syncthreads();
    return r;
}

// one lane's running (max, sum of exp(y - max)) over the y = x / T it has seen, plus what the picks need from the same sweep
struct BestLane {
    float m = -INFINITY, s = 0.f;
    float bx = -INFINITY;                                  // the best eligible column so far: its logit and index (-1: none)
    int bc = -1, n_elig = 0, bad = 0;
};

// The sum runs on y = x * (1 / T) and the hardware exponential: one multiply and ~4 instructions per column where the correctly
// rounded division and expf cost ~25, on 47 M columns per position.  What it costs in accuracy: y is within 1 ulp of x / T (1.9e-6 at
// |y| = 32, on terms that far from the maximum only if the row is nearly one-hot) and exp(d) for the d ~ 0 that carry the sum is good
// to ~1e-7 relative; the picks' own values are x / T - lse with the exact division (beam_row_best_kernel's last lines).
__device__ __forceinline__ void best_visit(BestLane& a, float x, int c, int unk, float inv_t) {
    const float y = x * inv_t;
    a.bad |= !(y < INFINITY);                          // NaN or +inf
    // one exp per column: exp(-|y - m|) is the new term under the old maximum, or the old sum's factor under the new one
    const float e = y == -INFINITY ? 0.f : __expf(-fabsf(y - a.m));    // (m = -inf so far: exp(-inf) = 0, and never inf - inf)
    if (y > a.m) { a.s = a.s * e + 1.f; a.m = y; }
    else a.s += e;
    // a thread meets its columns in ascending order, so "strictly larger" keeps the lower index among equal logits (-0.0 == +0.0)
    const bool el = c != unk && x > -INFINITY;
    a.n_elig += el;
    if (el && x > a.bx) { a.bx = x; a.bc = c; }
}

// The row's columns in the order every sweep of this file walks them: up to 3 scalars in front of the first 16-byte boundary, the
// aligned body four columns per load, the scalar tail.  fn(x, column)
template <typename F>
__device__ __forceinline__ void best_sweep(const float* __restrict__ row, int V, F fn) {
    const int tid = threadIdx.x;
    const int head = min(V, (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u));
    const int nvec = (V - head) >> 2;
    if (tid < head) fn(row[tid], tid);
    const float4* __restrict__ body = reinterpret_cast<const float4*>(row + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += BEST_NT) {
        const float4 v = body[i];
        const int c = head + 4 * i;
        fn(v.x, c); fn(v.y, c + 1); fn(v.z, c + 2); fn(v.w, c + 3);
    }
    const int c = head + 4 * nvec + tid;
    if (c < V) fn(row[c], c);
}

template <bool PR>
__global__ __launch_bounds__(BEST_NT) void beam_row_best_kernel(
    const float* __restrict__ logits, int ldl, int V, const float* __restrict__ gmax, int gm_ld, int n_groups, int gcols,
    int rows_per_img, int beam, float temperature, int unk, int step, const int32_t* __restrict__ first_pos,
    int32_t* __restrict__ pick_idx, float* __restrict__ pick_val, int32_t* __restrict__ err) {
    __shared__ best_key_t cand[BEST_CAP];
    __shared__ best_key_t red[BEST_NT];
    __shared__ best_key_t picks[DH_BEAM_MAX_BEAMS];
    __shared__ int glist[1024];
    __shared__ float wm[BEST_NT / 64], ws[BEST_NT / 64];
    __shared__ int wn[BEST_NT / 64];
    __shared__ best_key_t s_thr;
    __shared__ int s_cnt, s_ng;
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PR) {                                   // forced images, and all but the base row of an image at its first step
        const int fp = first_pos[rc / rows_per_img];
        if (step < fp || (step == fp && rc % rows_per_img != 0)) return;
    }
    const float* __restrict__ row = logits + (size_t)rc * ldl;
    int32_t* __restrict__ out_i = pick_idx + (size_t)rc * beam;
    float* __restrict__ out_v = pick_val + (size_t)rc * beam;

    // ---- pass 1
    BestLane a;
    const float inv_t = 1.f / temperature;
    best_sweep(row, V, [&](float x, int c) { best_visit(a, x, c, unk, inv_t); });
    const best_key_t top = a.bc >= 0 ? best_key(a.bx, a.bc, unk) : 0ull;
    if (tid == 0) { s_thr = 0ull; s_cnt = 0; s_ng = 0; }
    for (int j = tid; j < DH_BEAM_MAX_BEAMS; j += BEST_NT) picks[j] = 0ull;
    const int bad = __syncthreads_or(a.bad);              // (also orders the stores above)
    if (bad) {                                            // as the samplers: the flag and a finite dummy pick
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_NONFINITE);
        if (tid < beam) { out_i[tid] = 0; out_v[tid] = 0.f; }
        return;
    }
    // (max, sum) of the block: lanes -> wave -> the four waves, always in this order
    const float m_w = wave_max(a.m);
    const float s_w = wave_sum(a.s * expf(a.m - (m_w == -INFINITY ? 0.f : m_w)));      // (the few merges use the exact expf)
    const int n_w = wave_sum_i(a.n_elig);
    if (lane == 0) { wm[wave] = m_w; ws[wave] = s_w; wn[wave] = n_w; }
    red[tid] = top;
    __syncthreads();
    const float m_b = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    const float m_ref = m_b == -INFINITY ? 0.f : m_b;
    const float s_b = (ws[0] * expf(wm[0] - m_ref) + ws[1] * expf(wm[1] - m_ref)) + (ws[2] * expf(wm[2] - m_ref) + ws[3] * expf(wm[3] - m_ref));
    const int n_elig = (wn[0] + wn[1]) + (wn[2] + wn[3]);
    if (n_elig == 0) {                                    // (block-uniform) nothing finite but, at most, unk
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_ALL_FILTERED);
        if (tid < beam) { out_i[tid] = 0; out_v[tid] = 0.f; }
        return;
    }
    const float lse = m_b + logf(s_b);

    // ---- the bound: the beam-th largest thread best (keys are unique; fewer than `beam` threads saw an eligible column: no bound)
    {
        const best_key_t me = top;
        int r = 0;
        for (int j = 0; j < BEST_NT; ++j) r += red[j] > me;
        if (me != 0ull && r == beam - 1) s_thr = me;
    }
    __syncthreads();
    const best_key_t thr = s_thr;
    const float thr_x = thr != 0ull ? row[best_key_col(thr)] : -INFINITY;     // the bound's logit: a float compare in front of the keys

    // ---- pass 2: the columns that reach the bound
    auto take = [&](float x, int c) {
        if (x >= thr_x) {
            const best_key_t k = best_key(x, c, unk);
            if (k != 0ull && k >= thr) {
                const int at = atomicAdd(&s_cnt, 1);
                if (at < BEST_CAP) cand[at] = k;
            }
        }
    };
    if (gmax != nullptr) {
        // a group holds a column at the bound only if its maximum reaches the bound's logit
        const uint32_t thr_hi = (uint32_t)(thr >> 32);
        for (int g = tid; g < n_groups; g += BEST_NT)
            if (best_f2key(gmax[(size_t)rc * gm_ld + g]) >= thr_hi) glist[atomicAdd(&s_ng, 1)] = g;
        __syncthreads();
        const int ng = s_ng;
        for (int q = wave; q < ng; q += BEST_NT / 64) {   // one wave per group, one lane per column
            const int c = glist[q] * gcols + lane;
            if (lane < gcols && c < V) take(row[c], c);
        }
    } else {
        best_sweep(row, V, take);
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (cnt <= BEST_CAP) {
        for (int i = tid; i < cnt; i += BEST_NT) {
            const best_key_t me = cand[i];
            int r = 0;
            for (int j = 0; j < cnt; ++j) r += cand[j] > me;
            if (r < beam) picks[r] = me;
        }
    } else {
        // flat row: beam rounds of arg-max below the previous pick, over the row itself
        best_key_t last = ~0ull;
        for (int j = 0; j < beam; ++j) {
            best_key_t best = 0ull;
            for (int c = tid; c < V; c += BEST_NT) {
                const best_key_t k = best_key(row[c], c, unk);
                if (k < last && k > best) best = k;
            }
            best = best_block_max(best, red);
            if (tid == 0) picks[j] = best;
            if (best == 0ull) break;                       // (block-uniform) fewer than `beam` eligible columns
            last = best;
        }
    }
    __syncthreads();
    if (tid == 0 && n_elig < beam) atomicOr(err, DH_BEAM_ERR_TOO_FEW);      // dead beams: token 0 at -inf
    if (tid < beam) {
        const best_key_t k = picks[tid];
        const int c = best_key_col(k);
        out_i[tid] = k != 0ull ? c : 0;
        out_v[tid] = k != 0ull ? row[c] / temperature - lse : -INFINITY;
    }
}

// first_pos != NULL: the prompted phases (beam.hip, prompt_row_idle) with rows_per_img == beam.  group_max != NULL: [rows, gm_ld]
// maxima of n_groups groups of group_cols columns, else gm_ld / n_groups / group_cols are not looked at.
extern "C" int dh_beam_row_best(const float* logits, int ldl, int V, const float* group_max, int gm_ld, int n_groups, int group_cols,
                                int rows, int rows_per_img, int beam, float temperature, int unk_index, int step,
                                const int32_t* first_pos, int32_t* pick_idx, float* pick_val, int32_t* err, void* stream) {
    DH_REQUIRE(logits && pick_idx && pick_val && err && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V);
    DH_REQUIRE(beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && temperature > 0.f && temperature < INFINITY);
    DH_REQUIRE(!group_max || (n_groups > 0 && n_groups <= 1024 && gm_ld >= n_groups && group_cols > 0 && group_cols <= 64 &&
                              (long long)n_groups * group_cols >= V));
    DH_REQUIRE(!first_pos || (rows_per_img == beam && rows % beam == 0));
    DhProfScope prof("dh_beam_row_best", 0.0, 0.0, stream);
    if (first_pos)
        hipLaunchKernelGGL((beam_row_best_kernel<true>), dim3(rows), dim3(BEST_NT), 0, (hipStream_t)stream, logits, ldl, V, group_max, gm_ld,
                           n_groups, group_cols, rows_per_img, beam, temperature, unk_index, step, first_pos, pick_idx, pick_val, err);
    else
        hipLaunchKernelGGL((beam_row_best_kernel<false>), dim3(rows), dim3(BEST_NT), 0, (hipStream_t)stream, logits, ldl, V, group_max, gm_ld,
                           n_groups, group_cols, rows_per_img, beam, temperature, unk_index, step, first_pos, pick_idx, pick_val, err);
    DH_LAUNCH_CHECK();
}
