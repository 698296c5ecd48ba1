// return_logprobs: the model log-probability of every token a beam holds, log_softmax(x / T)[token] on the fp32 logits row the token was
// taken from -- behind the history edits and the bans, in front of the top-k / nucleus / unk filtering, normalised over every real
// column.  Three launches of their own; no sampler and no select is edited, and nothing follows the beam shuffles step by step:
//   pick   (in front of the select) : per logits row lse = logsumexp(x / T) in ONE sweep, then pick_lp[r, j] = x[r, pick_idx[r, j]] / T - lse
//                                     for the row's `beam` picks; an ended row gets zeros.  search="beam": a masked copy of pick_val.
//   record (behind the select)      : per beam row, slab c = step_index of two position-major tables: par_w[c, row] = the row it came
//                                     from, lp_w[c, row] = the pick_lp of the token the select wrote into it.
//   gather (behind the final draw)  : per kept beam one walk down the slabs along par_w, collecting lp_w for the beam's own columns.
// The sweep restates beam_best.hip's (16-byte loads, head / body / tail, an online (max, sum) per lane, lanes -> wave -> the four waves
// in a fixed tree, no float atomics): two runs are bit-identical and the error against fp64 is that kernel's (within 2e-5 at |x / T| <= 32).
#include "common.h"
#include "prof.h"

#define LP_NT 256

// one lane's running (max, sum of exp(y - max)) over the y = x / T it has seen (beam_best.hip, BestLane / best_visit, without the picks)
struct LpLane {
    float m = -INFINITY, s = 0.f;
    int bad = 0;
};

__device__ __forceinline__ void lp_visit(LpLane& a, float x, float inv_t) {
    const float y = x * inv_t;
    a.bad |= !(y < INFINITY);                          // NaN or +inf
    const float e = y == -INFINITY ? 0.f : __expf(-fabsf(y - a.m));    // (m = -inf so far: exp(-inf) = 0, and never inf - inf)
    if (y > a.m) { a.s = a.s * e + 1.f; a.m = y; }
    else a.s += e;
}

// the row's columns in beam_best.hip's order: up to 3 scalars in front of the first 16-byte boundary, the aligned body, the scalar tail
template <typename F>
__device__ __forceinline__ void lp_sweep(const float* __restrict__ row, int V, F fn) {
    const int tid = threadIdx.x;
    const int head = min(V, (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u));
    const int nvec = (V - head) >> 2;
    if (tid < head) fn(row[tid]);
    const float4* __restrict__ body = reinterpret_cast<const float4*>(row + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += LP_NT) {
        const float4 v = body[i];
        fn(v.x); fn(v.y); fn(v.z); fn(v.w);
    }
    const int c = head + 4 * nvec + tid;
    if (c < V) fn(row[c]);
}

// PR: the prompted phases (beam.hip, prompt_row_idle): a forced image's rows, and all but the base row of an image at its first step,
// are neither read nor written.  vals != NULL (search="beam"): no sweep, pick_lp = the bits dh_beam_row_best left in pick_val.
template <bool PR>
__global__ __launch_bounds__(LP_NT) void beam_pick_logprobs_kernel(
    const float* __restrict__ logits, int ldl, int V, int rows_per_img, int beam, float temperature, int step,
    const int32_t* __restrict__ first_pos, const uint8_t* __restrict__ ended, const int32_t* __restrict__ pick_idx,
    const float* __restrict__ vals, float* __restrict__ pick_lp) {
    __shared__ float wm[LP_NT / 64], ws[LP_NT / 64];
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PR) {
        const int fp = first_pos[rc / rows_per_img];
        if (step < fp || (step == fp && rc % rows_per_img != 0)) return;
    }
    float* __restrict__ out = pick_lp + (size_t)rc * beam;
    // the beam-state row of logits row rc: a dense first step's compact rows sit at img * beam
    const size_t trow = rows_per_img == 1 ? (size_t)rc * beam : (size_t)rc;
    if (ended[trow]) {                                    // (block-uniform) an ended beam draws nothing: its one candidate adds 0
        if (tid < beam) out[tid] = 0.f;
        return;
    }
    if (vals != nullptr) {
        if (tid < beam) out[tid] = vals[(size_t)rc * beam + tid];
        return;
    }
    const float* __restrict__ row = logits + (size_t)rc * ldl;
    LpLane a;
    const float inv_t = 1.f / temperature;
    lp_sweep(row, V, [&](float x) { lp_visit(a, x, inv_t); });
    const int bad = __syncthreads_or(a.bad);
    // (max, sum) of the block: lanes -> wave -> the four waves, always in this order
    const float m_w = wave_max(a.m);
    const float s_w = wave_sum(a.s * expf(a.m - (m_w == -INFINITY ? 0.f : m_w)));      // (the few merges use the exact expf)
    if (lane == 0) { wm[wave] = m_w; ws[wave] = s_w; }
    __syncthreads();
    const float m_b = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    if (bad || m_b == -INFINITY) {                        // (block-uniform) the row step flags these rows; here: zeros, never NaN
        if (tid < beam) out[tid] = 0.f;
        return;
    }
    const float s_b = (ws[0] * expf(wm[0] - m_b) + ws[1] * expf(wm[1] - m_b)) + (ws[2] * expf(wm[2] - m_b) + ws[3] * expf(wm[3] - m_b));
    const float lse = m_b + logf(s_b);
    if (tid < beam) {
        const int c = pick_idx[(size_t)rc * beam + tid];
        out[tid] = (c >= 0 && c < V) ? row[c] / temperature - lse : 0.f;     // (the exact division, as dh_beam_row_best's pick_val)
    }
}

extern "C" int dh_beam_pick_logprobs(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam, float temperature, int step,
                                     const int32_t* first_pos, const uint8_t* ended, const int32_t* pick_idx, const float* pick_val,
                                     int from_vals, float* pick_lp, void* stream) {
    DH_REQUIRE(ended && pick_lp && rows > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && (rows_per_img == 1 || rows_per_img == beam));
    DH_REQUIRE(from_vals ? pick_val != nullptr : (logits && pick_idx && V > 0 && ldl >= V && temperature > 0.f && temperature < INFINITY));
    DH_REQUIRE(!first_pos || (rows_per_img == beam && rows % beam == 0));
    DhProfScope prof("dh_beam_pick_logprobs", 0.0, from_vals ? 8.0 * rows * beam : 4.0 * rows * V, stream);
    const float* vals = from_vals ? pick_val : nullptr;
    if (first_pos)
        hipLaunchKernelGGL((beam_pick_logprobs_kernel<true>), dim3(rows), dim3(LP_NT), 0, (hipStream_t)stream, logits, ldl, V, rows_per_img,
                           beam, temperature, step, first_pos, ended, pick_idx, vals, pick_lp);
    else
        hipLaunchKernelGGL((beam_pick_logprobs_kernel<false>), dim3(rows), dim3(LP_NT), 0, (hipStream_t)stream, logits, ldl, V, rows_per_img,
                           beam, temperature, step, first_pos, ended, pick_idx, vals, pick_lp);
    DH_LAUNCH_CHECK();
}

// One thread per beam row.  An image that takes no step -- forced (step_index < first_pos[img]) or done before this step -- writes
// nothing: its slab stays identity / 0.  write_pos >= tok_ld (the Transformer decoders' last step, which re-draws the beams and writes
// no column): parents only.
__global__ __launch_bounds__(256) void beam_record_logprobs_kernel(
    const int32_t* __restrict__ tokens, int tok_ld, const int32_t* __restrict__ parent, const uint8_t* __restrict__ done,
    const int32_t* __restrict__ end_step, const int32_t* __restrict__ pick_idx, const float* __restrict__ pick_lp, int rows, int beam,
    int first, const int32_t* __restrict__ first_pos, int write_pos, int step_index, float* __restrict__ lp_w, int32_t* __restrict__ par_w) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int img = row / beam;
    if (first_pos) {
        const int fp = first_pos[img];
        if (step_index < fp) return;
        first = step_index == fp;
    }
    if (done[img] && end_step[img] < step_index) return;
    const int par = parent[row];
    const size_t at = (size_t)step_index * rows + row;
    par_w[at] = (par >= 0 && par < rows) ? par : row;
    if (write_pos >= tok_ld) return;
    // the logits row the token came from: the parent; at a first step the image's compact row (dense) or its base row (prompted)
    const int prow = first ? (first_pos ? img * beam : img) : par;
    float v = 0.f;
    if (prow >= 0 && prow < rows) {
        const int tok = tokens[(size_t)row * tok_ld + write_pos];
        for (int j = 0; j < beam; ++j)
            if (pick_idx[(size_t)prow * beam + j] == tok) { v = pick_lp[(size_t)prow * beam + j]; break; }
    }
    lp_w[at] = v;
}

extern "C" int dh_beam_record_logprobs(const int32_t* tokens, int tok_ld, const int32_t* parent, const uint8_t* done, const int32_t* end_step,
                                       const int32_t* pick_idx, const float* pick_lp, int n_img, int beam, int first,
                                       const int32_t* first_pos, int write_pos, int step_index, int n_pos, float* lp_w, int32_t* par_w,
                                       void* stream) {
    DH_REQUIRE(tokens && parent && done && end_step && pick_idx && pick_lp && lp_w && par_w);
    DH_REQUIRE(n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && tok_ld > 0 && write_pos >= 0 && step_index >= 0 && step_index < n_pos);
    const int rows = n_img * beam;
    DhProfScope prof("dh_beam_record_logprobs", 0.0, 16.0 * rows, stream);
    hipLaunchKernelGGL(beam_record_logprobs_kernel, dim3(dh_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, tokens, tok_ld, parent, done,
                       end_step, pick_idx, pick_lp, rows, beam, first, first_pos, write_pos, step_index, lp_w, par_w);
    DH_LAUNCH_CHECK();
}

// One thread per kept beam: from r = i * beam + index[i, j] down the slabs, out[i, j, c] = lp_w[c, r] for the beam's own columns (from
// the image's first generated column up to len[i, j]), then r = par_w[c, r].  Every slab is walked, the ones past the beam's length and
// the step that wrote no column included, so the parents stay right; every other element of out is 0.
__global__ __launch_bounds__(256) void beam_gather_logprobs_kernel(
    const float* __restrict__ lp_w, const int32_t* __restrict__ par_w, const int32_t* __restrict__ index, const int32_t* __restrict__ len,
    int rows, int beam, int T, int n_pos, int pos, const int32_t* __restrict__ first_pos, float* __restrict__ out) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= rows) return;
    const int img = slot / beam;
    const int p0 = first_pos ? first_pos[img] : pos, n = len[slot];
    float* __restrict__ dst = out + (size_t)slot * T;
    int r = img * beam + min(max(index[slot], 0), beam - 1);
    for (int c = n_pos - 1; c >= 0; --c) {
        const size_t at = (size_t)c * rows + r;
        if (c < T) dst[c] = (c >= p0 && c < n) ? lp_w[at] : 0.f;
        const int p = par_w[at];
        if (p >= 0 && p < rows) r = p;                    // (never a foreign read, whatever the table holds)
    }
}

extern "C" int dh_beam_gather_logprobs(const float* lp_w, const int32_t* par_w, const int32_t* index, const int32_t* len, int n_img, int beam,
                                       int T, int n_pos, int pos, const int32_t* first_pos, float* out, void* stream) {
    DH_REQUIRE(lp_w && par_w && index && len && out && n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS);
    DH_REQUIRE(T > 0 && T <= n_pos && pos >= 0);
    const int rows = n_img * beam;
    DhProfScope prof("dh_beam_gather_logprobs", 0.0, 8.0 * rows * n_pos + 4.0 * rows * T, stream);
    hipLaunchKernelGGL(beam_gather_logprobs_kernel, dim3(dh_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, lp_w, par_w, index, len, rows,
                       beam, T, n_pos, pos, first_pos, out);
    DH_LAUNCH_CHECK();
}
