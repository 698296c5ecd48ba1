// Device-side beam-search step (deephumor/models/beam.py), batched over images: no host sync and no
// torch.multinomial in the token loop.
//   beam_row_sample : per (image, beam) row -- k-th-largest threshold by 4-pass radix select over the
//                     logits row (L2-resident after the vocabulary GEMM wrote it), survivor
//                     compaction into LDS, temperature softmax, Exp(1)-race draw of `beam` tokens
//                     (== CPU torch.multinomial without replacement), log-softmax over the picks.
//   beam_select     : per image -- candidate list with ended-beam dedup, second race, in-place
//                     rewrite of tokens / scores / ended flags / KV-ancestor table / parent rows.
//   beam_finalize   : per image -- final single draw and output copy.
#include "common.h"
#include "prof.h"

#define CAP DH_BEAM_MAX_SURVIVORS

// order-preserving float -> uint key (larger float <=> larger key; -0.0 and +0.0 share ONE key, as they compare equal in the
// reference's `logits < threshold` (beam.py:34): with distinct keys a row whose k-th largest logit is a zero dropped the zeros of the
// other sign that torch keeps as ties -- found by tools/fuzz_sampler.py on quantised logits).  A NaN of EITHER sign gets the largest
// key, as torch.topk ranks it (beam.py:32): it is then always among a row's survivors and the row flags DH_BEAM_ERR_NONFINITE where
// the reference's torch.multinomial raises -- with the plain bit trick a NaN whose sign bit is set ordered below -inf, fell out of
// the top-k and the row was drawn without a flag.
__device__ __forceinline__ uint32_t f2key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}


// Picks the radix digit holding the k-th largest key: the digit d with (#keys in digits > d) < k <= (... >= d).
// Parallel suffix sum over the 256 bins (wave shuffles + 4 wave totals) instead of a serial scan whose
// dependent LDS reads cost ~10 us per pass.  Must be called by all threads of the block; threads
// 0..255 own one bin each.  `bins` may be 1 or 4 histograms of 256 (summed).
__device__ __forceinline__ void radix_pick_digit(const int* hist, int n_hist, int shift, uint32_t prefix,
                                                 uint32_t* s_prefix, int* s_k, int* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = *s_k;
    int c = 0, suf = 0;
    if (tid < 256) {
        for (int h = 0; h < n_hist; ++h) c += hist[h * 256 + tid];
        // inclusive suffix sum inside the wave (towards higher lanes): DPP row_shl scan inside the 16-lane rows (a lane
        // shifted in from beyond the row end reads 0), then the totals of the higher rows through v_readlane
        suf = c;
        suf += __builtin_amdgcn_update_dpp(0, suf, 0x101, 0xF, 0xF, true);
        suf += __builtin_amdgcn_update_dpp(0, suf, 0x102, 0xF, 0xF, true);
        suf += __builtin_amdgcn_update_dpp(0, suf, 0x104, 0xF, 0xF, true);
        suf += __builtin_amdgcn_update_dpp(0, suf, 0x108, 0xF, 0xF, true);
        {
            const int t1 = __builtin_amdgcn_readlane(suf, 16), t2 = __builtin_amdgcn_readlane(suf, 32), t3 = __builtin_amdgcn_readlane(suf, 48);
            const int row = lane >> 4;
            suf += row == 0 ? t1 + t2 + t3 : row == 1 ? t2 + t3 : row == 2 ? t3 : 0;
        }
        if (lane == 0) wtot[wave] = suf;
    }
    __syncthreads();
    if (tid < 256) {
        int above = suf - c;                       // bins above me inside my wave
        for (int w = wave + 1; w < 4; ++w) above += wtot[w];
        if (above < k && k <= above + c) { *s_prefix = prefix | ((uint32_t)tid << shift); *s_k = k - above; }
    }
    __syncthreads();
}

// lanes of one wave exchanging data through LDS without a workgroup barrier: keep the compiler from moving LDS accesses
// across the hand-over (the hardware executes a wave's LDS operations in order)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// DPP move with zero fill: row_shr:n (CTRL 0x110 + n) hands lane l the value of lane l - n of its 16-lane row, 0.f before the row start
template <int CTRL>
__device__ __forceinline__ float dpp_shr0(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

__device__ __forceinline__ float block_reduce_256(float v, float* red, bool is_max) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = is_max ? fmaxf(red[tid], red[tid + s]) : red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

template <int NT>
__device__ __attribute__((noinline)) void row_overflow(const float* __restrict__ row, int V, uint32_t thr, int rc, int ldl, int rows_per_img, int beam,
                             float temperature, int unk, const float* __restrict__ noise, uint64_t seed,
                             const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* __restrict__ pick_idx,
                             float* __restrict__ pick_val, float* sq, int* si, int* picks, int32_t* __restrict__ err);
__device__ __forceinline__ void pick_store(int32_t* pi, float* pv, size_t at, int32_t idx, float val);

// softmax over a row's survivors: max m, sum s of exp(x - m).  Finite logits give a finite m and s >= 1 (the maximum contributes exp(0));
// a NaN among them makes s NaN, +inf makes m = +inf and s NaN, only-NaN survivors leave m = -inf: the reference's torch.multinomial raises
// on such a row ("probability tensor contains either `inf`, `nan` or element < 0", beam.py:46) -- the samplers flag DH_BEAM_ERR_NONFINITE
// and hand on a finite dummy pick, so that nothing downstream indexes with garbage
__device__ __forceinline__ bool dh_softmax_nonfinite(float m, float s) { return !(s >= 1.0f) || !(fabsf(m) < INFINITY); }

// Prompted launches (the *_prompted entry points; PR = true instantiations): every image of the batch brings its own prompt length
// first_pos[img] and `step` is the launch's absolute position, so the image is in one of three phases --
//   step <  first_pos[img]  forced: the position's token is the prompt's; nothing is drawn, the row's logits are not read;
//   step == first_pos[img]  first : the image's logical row img * beam is its single source row (rnn_models.py:73-103,
//                                   transformers.py:517-545) -- it draws with row index 0, exactly as the dense first step does;
//   step >  first_pos[img]  normal: today's step.
// One workgroup owns one row, so the test is workgroup-uniform and the idle rows leave before the first barrier.
__device__ __forceinline__ bool prompt_row_idle(const int32_t* __restrict__ first_pos, int rc, int rows_per_img, int step) {
    const int fp = first_pos[rc / rows_per_img];
    return step < fp || (step == fp && rc % rows_per_img != 0);
}

struct RowLds {
    int* idx_a; int* idx_b; float* val_a; float* val_b; float* qv; float* red; int* picks; int* s_cnt; uint32_t* s_thr;
};
template <int NT, bool NU>
__device__ __forceinline__ void row_tail(const RowLds& L, int rc, int ldl, int rows_per_img, int beam, int top_k,
                                         float temperature, int unk, const float* __restrict__ noise, uint64_t seed,
                                         const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* __restrict__ pick_idx,
                                         float* __restrict__ pick_val, int32_t* __restrict__ err, float top_p);

// NU (dh_beam_row_sample_nucleus; the same parameter on the two pre-filtered kernels below): the draw runs over the row's NUCLEUS --
// the survivors whose exclusive prefix of p, in the order (p descending, token index ascending), is < top_p, and never fewer than
// `beam` of them (row_tail).  The NU = false instantiations are the kernels of every other entry point: top_p is not read there.
template <bool PR, bool NU = false>
__global__ __launch_bounds__(256) void beam_row_sample_kernel(
    const float* __restrict__ logits, int ldl, int V, int rows_per_img, int beam, int top_k,
    float temperature, int unk, const float* __restrict__ noise, uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step,
    int32_t* __restrict__ pick_idx, float* __restrict__ pick_val, int32_t* __restrict__ err, const int32_t* __restrict__ first_pos,
    float top_p) {
    __shared__ int hist[4][256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k, s_cnt, wtot[4];
    __shared__ __attribute__((aligned(16))) int idx_a[CAP], idx_b[CAP];
    __shared__ __attribute__((aligned(16))) float val_a[CAP], val_b[CAP], qv[CAP];
    __shared__ float red[256];
    __shared__ int picks[DH_BEAM_MAX_BEAMS];

    const int rc = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if constexpr (PR) { if (prompt_row_idle(first_pos, rc, rows_per_img, step)) return; }
    const float* row = logits + (size_t)rc * ldl;

    // ---- k-th largest by MSB-first radix select on the order-preserving key --------------------
    if (tid == 0) { s_prefix = 0u; s_k = top_k; s_cnt = 0; }
    uint32_t mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 1024; i += 256) (&hist[0][0])[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (int i = tid; i < V; i += 256) {
            const uint32_t key = f2key(row[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[wave][(key >> shift) & 255u], 1);
        }
        __syncthreads();
        radix_pick_digit(&hist[0][0], 4, shift, prefix, &s_prefix, &s_k, wtot);
        mask |= 0xFFu << shift;
    }
    const uint32_t thr = s_prefix;

    // ---- survivors: logit >= threshold (ties kept, beam.py:34), unk always dropped (:35) -------
    for (int i = tid; i < V; i += 256) {
        const float v = row[i];
        if (f2key(v) >= thr && i != unk) {
            const int p = atomicAdd(&s_cnt, 1);
            if (p < CAP) { idx_a[p] = i; val_a[p] = v; }
        }
    }
    __syncthreads();
    int n = s_cnt;
    if constexpr (NU) {
        // No nucleus over a row in global memory: more survivors than the candidate buffers hold is DH_BEAM_ERR_OVERFLOW here too
        // (row_overflow is not entered).  Otherwise the common tail: its threshold search finds no better value than the preset
        // one when <unk> has already left the candidates (every candidate is >= thr, so thr is the only key it can write).
        __shared__ uint32_t s_thr;
        if (n > CAP) {
            if (tid == 0) atomicOr(err, DH_BEAM_ERR_OVERFLOW);
            if (tid < beam) { pick_idx[(size_t)rc * beam + tid] = 0; pick_val[(size_t)rc * beam + tid] = 0.f; }
            return;
        }
        if (tid == 0) s_thr = thr;
        __syncthreads();
        const RowLds L{idx_a, idx_b, val_a, val_b, qv, red, picks, &s_cnt, &s_thr};
        row_tail<256, true>(L, rc, ldl, rows_per_img, beam, top_k, temperature, unk, noise, seed, seed_ptr, img0, step, pick_idx, pick_val,
                            err, top_p);
        return;
    }
    if (n > CAP) {                   // more ties at the threshold than the candidate buffers hold: the draw over the row itself
        row_overflow<256>(row, V, thr, rc, ldl, rows_per_img, beam, temperature, unk, noise, seed, seed_ptr, img0, step, pick_idx, pick_val,
                          qv, idx_b, picks, err);
        return;
    }
    if (n == 0) {
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_ALL_FILTERED);
        if (tid < beam) { pick_idx[(size_t)rc * beam + tid] = 0; pick_val[(size_t)rc * beam + tid] = 0.f; }
        return;
    }
    // deterministic order: sort by token index (rank sort, n is ~top_k)
    for (int i = tid; i < n; i += 256) {
        const int me = idx_a[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += (idx_a[j] < me);
        idx_b[r] = me; val_b[r] = val_a[i];
    }
    __syncthreads();

    // ---- p = softmax(filtered / T);  q = p / Exp(1) noise -------------------------------------
    float m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, val_b[i] / temperature);
    m = block_reduce_256(m, red, true);
    float s = 0.f;
    for (int i = tid; i < n; i += 256) { const float e = expf(val_b[i] / temperature - m); qv[i] = e; s += e; }
    s = block_reduce_256(s, red, false);
    if (dh_softmax_nonfinite(m, s)) {                  // (block-uniform)
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_NONFINITE);
        if (tid < beam) { pick_idx[(size_t)rc * beam + tid] = 0; pick_val[(size_t)rc * beam + tid] = 0.f; }
        return;
    }
    const int img = rc / rows_per_img, rin = rc % rows_per_img;
    for (int i = tid; i < n; i += 256) {
        const float nz = noise ? noise[(size_t)rc * ldl + idx_b[i]]
                               : philox_exp1(seed ^ (seed_ptr ? *seed_ptr : 0ull), (uint32_t)(img0 + img), (uint32_t)step, 0u, (uint32_t)rin, (uint32_t)idx_b[i]);
        qv[i] = (qv[i] / s) / nz;
    }
    if (tid < DH_BEAM_MAX_BEAMS) picks[tid] = -1;
    __syncthreads();
    // top-`beam` of q, descending; ties -> lower token index first (argmax semantics for beam == 1)
    for (int i = tid; i < n; i += 256) {
        const float me = qv[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += (qv[j] > me) || (qv[j] == me && j < i);
        if (r < beam) picks[r] = i;
    }
    __syncthreads();
    if (tid == 0) {
        // fewer positive-probability tokens than beams: a survivor at -inf (a threshold of -inf keeps them all) is a dead pick too
        int n_live = 0;
        for (int b = 0; b < beam; ++b) n_live += picks[b] >= 0 && val_b[picks[b]] > -INFINITY;
        if (n_live < beam) atomicOr(err, DH_BEAM_ERR_TOO_FEW);
        // log_softmax over the gathered (un-tempered) logits of the picks (beam.py:79)
        float mx = -INFINITY;
        for (int b = 0; b < beam; ++b) if (picks[b] >= 0) mx = fmaxf(mx, val_b[picks[b]]);
        float se = 0.f;
        for (int b = 0; b < beam; ++b) if (picks[b] >= 0) se += expf(val_b[picks[b]] - mx);
        const float lse = logf(se);
        for (int b = 0; b < beam; ++b) {
            const int pi = picks[b];
            pick_idx[(size_t)rc * beam + b] = pi >= 0 ? idx_b[pi] : 0;
            pick_val[(size_t)rc * beam + b] = pi >= 0 ? (val_b[pi] - mx) - lse : -INFINITY;
        }
    }
}


// Exact candidate set of a row for the pre-filtered kernels' overflow case (their bound let more than CAP values
// through -- flat or heavily tied logits): k-th largest key by the 4-pass MSB-first radix select over the whole row
// (as beam_row_sample_kernel), then every value >= it is compacted into idx_a / val_a (*s_cnt = their number; more
// than CAP only if that many logits tie at the threshold).  hist: 4 x 256 ints.  Block-uniform call; synchronised on return.
template <int NT>
__device__ void radix_row_candidates(const float* __restrict__ row, int V, int top_k, int* hist, uint32_t* s_prefix, int* s_k,
                                     int* s_cnt, int* wtot, int* idx_a, float* val_a) {
    const int tid = threadIdx.x, hw = (tid >> 6) & 3;
    __syncthreads();
    if (tid == 0) { *s_prefix = 0u; *s_k = top_k; *s_cnt = 0; }
    uint32_t mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 1024; i += NT) hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = *s_prefix;
        for (int i = tid; i < V; i += NT) {
            const uint32_t key = f2key(row[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[hw * 256 + ((key >> shift) & 255u)], 1);
        }
        __syncthreads();
        radix_pick_digit(hist, 4, shift, prefix, s_prefix, s_k, wtot);
        mask |= 0xFFu << shift;
    }
    const uint32_t thr = *s_prefix;
    for (int i = tid; i < V; i += NT) {
        const float v = row[i];
        if (f2key(v) >= thr) {
            const int p = atomicAdd(s_cnt, 1);
            if (p < CAP) { idx_a[p] = i; val_a[p] = v; }
        }
    }
    __syncthreads();
}

// ---- single-pass variant --------------------------------------------------------------------------
// The logits row is read from HBM exactly ONCE, straight into registers (512 threads x EPT values,
// every load issued up front).  A valid lower bound of the k-th largest value is the k-th largest of
// the 512 per-thread maxima (k <= 512): at least k elements are >= it.  Everything >= that bound
// (about top_k..2*top_k values on real logits) is compacted into LDS and the exact threshold,
// the survivors and the draws are computed there.  If more than CAP values pass the bound (flat / tied
// logits) the kernel re-derives the exact candidate set in place with radix_row_candidates.
__device__ __forceinline__ void pick_store(int32_t* pi, float* pv, size_t at, int32_t idx, float val) { pi[at] = idx; pv[at] = val; }

// More than CAP logits of a row tie at (or exceed) its top-k threshold -- flat or constant logits -- so the survivors do not fit the
// LDS candidate buffers: the draw runs over the ROW in global memory instead (beam.py:32-48 unchanged: every logit >= the threshold
// survives, <unk> dropped, softmax / T, `beam` winners of p / Exp(1), ties to the lower index).  `beam` block-wide arg-max rounds over
// V elements: slow and exact, for a case that trained models do not produce.  sq / si: NT floats / ints of LDS scratch.
// Only the general kernel (beam_row_sample_kernel) carries it: inside the pre-filtered kernels of the hot path it cost 1-2 % of the C2 step
// even as a never-taken call (registers 44 -> 88, scratch set-up), so those still flag DH_BEAM_ERR_OVERFLOW and the host repeats the batch
// through dh_beam_row_sample_exact (deephumor_amd/models/beam.py).
template <int NT>
__device__ __attribute__((noinline)) void row_overflow(const float* __restrict__ row, int V, uint32_t thr, int rc, int ldl, int rows_per_img, int beam,
                             float temperature, int unk, const float* __restrict__ noise, uint64_t seed,
                             const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* __restrict__ pick_idx,
                             float* __restrict__ pick_val, float* sq, int* si, int* picks, int32_t* __restrict__ err) {
    const int tid = threadIdx.x;
    // (every loop rolled: this path must not raise the register count of the kernels that call it -- at 116 VGPRs instead of 44 the
    //  group-guided sampler lost a wave of occupancy, its 1,280 workgroups no longer fitted the chip in one round: +9 us per launch)
    float m = -INFINITY;
#pragma unroll 1
    for (int i = tid; i < V; i += NT) { const float v = row[i]; if (f2key(v) >= thr && i != unk) m = fmaxf(m, v / temperature); }
    __syncthreads();
    sq[tid] = m;
    __syncthreads();
#pragma unroll 1
    for (int st = NT / 2; st > 0; st >>= 1) { if (tid < st) sq[tid] = fmaxf(sq[tid], sq[tid + st]); __syncthreads(); }
    m = sq[0];
    __syncthreads();
    float part = 0.f;
#pragma unroll 1
    for (int i = tid; i < V; i += NT) { const float v = row[i]; if (f2key(v) >= thr && i != unk) part += expf(v / temperature - m); }
    sq[tid] = part;
    __syncthreads();
#pragma unroll 1
    for (int st = NT / 2; st > 0; st >>= 1) { if (tid < st) sq[tid] += sq[tid + st]; __syncthreads(); }
    const float s = sq[0];
    if (dh_softmax_nonfinite(m, s)) {                  // (block-uniform)
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_NONFINITE);
        if (tid < beam) pick_store(pick_idx, pick_val, (size_t)rc * beam + tid, 0, 0.f);
        return;
    }
    const int img = rc / rows_per_img, rin = rc % rows_per_img;
    const uint64_t sd = seed ^ (seed_ptr ? *seed_ptr : 0ull);
#pragma unroll 1
    for (int round = 0; round < beam; ++round) {
        float bq = -1.f; int bi = 0x7FFFFFFF;
#pragma unroll 1
        for (int i = tid; i < V; i += NT) {
            const float v = row[i];
            if (!(f2key(v) >= thr && i != unk)) continue;
            bool taken = false;
#pragma unroll 1
            for (int j = 0; j < round; ++j) taken |= picks[j] == i;
            if (taken) continue;
            const float nz = noise ? noise[(size_t)rc * ldl + i] : philox_exp1(sd, (uint32_t)(img0 + img), (uint32_t)step, 0u, (uint32_t)rin, (uint32_t)i);
            const float q = (expf(v / temperature - m) / s) / nz;
            if (q > bq) { bq = q; bi = i; }             // ascending i: the first (lowest) index wins a tie
        }
        __syncthreads();
        sq[tid] = bq; si[tid] = bi;
        __syncthreads();
#pragma unroll 1
        for (int st = NT / 2; st > 0; st >>= 1) {
            if (tid < st) {
                const float oq = sq[tid + st]; const int oi = si[tid + st];
                if (oq > sq[tid] || (oq == sq[tid] && oi < si[tid])) { sq[tid] = oq; si[tid] = oi; }
            }
            __syncthreads();
        }
        if (tid == 0) picks[round] = si[0];
        __syncthreads();
    }
    if (tid == 0) {                                    // log_softmax over the gathered (un-tempered) logits of the picks (beam.py:79)
        float mx = -INFINITY;
        int n_live = 0;                                  // (more than CAP survivors, yet fewer than `beam` above -inf: dead picks)
#pragma unroll 1
        for (int b = 0; b < beam; ++b) { mx = fmaxf(mx, row[picks[b]]); n_live += row[picks[b]] > -INFINITY; }
        if (n_live < beam) atomicOr(err, DH_BEAM_ERR_TOO_FEW);
        float se = 0.f;
#pragma unroll 1
        for (int b = 0; b < beam; ++b) se += expf(row[picks[b]] - mx);
        const float lse = logf(se);
#pragma unroll 1
        for (int b = 0; b < beam; ++b) pick_store(pick_idx, pick_val, (size_t)rc * beam + b, picks[b], (row[picks[b]] - mx) - lse);
    }
}

// Common tail of the row kernels.  On entry idx_a/val_a hold *s_cnt candidates that include every value >= the
// row's k-th largest (block-synchronised).  Exact threshold -> survivors (ties kept, unk dropped) -> index
// order -> softmax(filtered / T) -> Exp(1) race for `beam` picks -> log_softmax over the picks.
// NU: between softmax and race the nucleus mask -- p = e / s in index order (val_b), rank sort by (p descending, index ascending)
// (idx_b[rank] = index-order slot), exclusive block scan of p in that order, and a survivor at sorted position j whose prefix is
// >= top_p leaves the race (q = -1 < every real q) unless j < beam.  The noise stays indexed by token id.
template <int NT, bool NU>
__device__ __forceinline__ void row_tail(const RowLds& L, int rc, int ldl, int rows_per_img, int beam, int top_k,
                                         float temperature, int unk, const float* __restrict__ noise, uint64_t seed,
                                         const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* __restrict__ pick_idx,
                                         float* __restrict__ pick_val, int32_t* __restrict__ err, float top_p) {
    const int tid = threadIdx.x;
    int* idx_a = L.idx_a; int* idx_b = L.idx_b; float* val_a = L.val_a; float* val_b = L.val_b;
    float* qv = L.qv; float* red = L.red; int* picks = L.picks;
#define s_cnt (*L.s_cnt)
#define s_thr (*L.s_thr)
    int n0 = s_cnt;
    __syncthreads();                // every wave has read the candidate count before thread 0 resets it below
    if (n0 > CAP) { if (tid == 0) atomicOr(err, DH_BEAM_ERR_OVERFLOW); n0 = CAP; }
    // exact k-th largest among the candidates: the value whose "strictly greater" count is < k <= "greater or equal"
    for (int i = tid; i < n0; i += NT) {
        const uint32_t me = f2key(val_a[i]);
        int gt = 0, ge = 0;
        for (int j = 0; j < n0; ++j) { const uint32_t o = f2key(val_a[j]); gt += (o > me); ge += (o >= me); }
        if (gt < top_k && top_k <= ge) s_thr = me;      // all writers agree on the value
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t thr = s_thr;
    // survivors: >= threshold (ties kept), unk dropped
    for (int i = tid; i < n0; i += NT) {
        if (f2key(val_a[i]) >= thr && idx_a[i] != unk) {
            const int p = atomicAdd(&s_cnt, 1);
            idx_b[p] = idx_a[i]; val_b[p] = val_a[i];
        }
    }
    __syncthreads();
    const int n = s_cnt;
    if (n == 0) {
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_ALL_FILTERED);
        if (tid < beam) pick_store(pick_idx, pick_val, (size_t)rc * beam + tid, 0, 0.f);
        return;
    }
    // deterministic order: sort survivors by token index
    for (int i = tid; i < n; i += NT) {
        const int me = idx_b[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += (idx_b[j] < me);
        idx_a[r] = me; val_a[r] = val_b[i];
    }
    __syncthreads();
    // block max / sum: wave shuffles, then the NT/64 wave partials through LDS (2 barriers each instead of a log2(NT) tree)
    constexpr int NWV = NT / 64;
    float m = -INFINITY;
    for (int i = tid; i < n; i += NT) m = fmaxf(m, val_a[i] / temperature);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < n; i += NT) { const float e = expf(val_a[i] / temperature - m); qv[i] = e; s += e; }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = red[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) s += red[w];      // same order in every thread: one value for the whole block
    if (dh_softmax_nonfinite(m, s)) {                  // (block-uniform)
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_NONFINITE);
        if (tid < beam) pick_store(pick_idx, pick_val, (size_t)rc * beam + tid, 0, 0.f);
        return;
    }
    const int img = rc / rows_per_img, rin = rc % rows_per_img;
    for (int i = tid; i < n; i += NT) {
        const float nz = noise ? noise[(size_t)rc * ldl + idx_a[i]]
                               : philox_exp1(seed ^ (seed_ptr ? *seed_ptr : 0ull), (uint32_t)(img0 + img), (uint32_t)step, 0u, (uint32_t)rin, (uint32_t)idx_a[i]);
        if constexpr (NU) val_b[i] = qv[i] / s;
        qv[i] = (qv[i] / s) / nz;
    }
    if (tid < DH_BEAM_MAX_BEAMS) picks[tid] = -1;
    __syncthreads();
    if constexpr (NU) {
        // rank sort like the index sort above (n is ~top_k: every thread reads the same address, an LDS broadcast)
        for (int i = tid; i < n; i += NT) {
            const float me = val_b[i];
            int r = 0;
            for (int j = 0; j < n; ++j) r += (val_b[j] > me) || (val_b[j] == me && j < i);
            idx_b[r] = i;
        }
        __syncthreads();
        // exclusive scan of p over the sorted positions: thread t owns positions [t * IPT, (t + 1) * IPT) -- its own run serially,
        // the runs of a wave by DPP row_shr inside the 16-lane rows (a lane shifted in from before the row start reads 0) plus
        // the totals of the lower rows through v_readlane, the waves through their totals in LDS
        constexpr int IPT = CAP / NT;
        static_assert(IPT * NT == CAP && IPT >= 1, "one contiguous run of sorted positions per thread");
        const int lane = tid & 63, wave = tid >> 6;
        float loc[IPT], run = 0.f;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const int pos = tid * IPT + k;
            loc[k] = pos < n ? val_b[idx_b[min(pos, n - 1)]] : 0.f;
            run += loc[k];
        }
        float inc = run;
        inc += dpp_shr0<0x111>(inc); inc += dpp_shr0<0x112>(inc); inc += dpp_shr0<0x114>(inc); inc += dpp_shr0<0x118>(inc);
        const float t0 = lane_get(inc, 15), t1 = lane_get(inc, 31), t2 = lane_get(inc, 47), t3 = lane_get(inc, 63);
        const int drow = lane >> 4;
        float pre = (drow == 0 ? 0.f : drow == 1 ? t0 : drow == 2 ? t0 + t1 : (t0 + t1) + t2) + dpp_shr0<0x111>(inc);
        if (lane == 0) red[wave] = ((t0 + t1) + t2) + t3;
        __syncthreads();
        float below = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) below += w < wave ? red[w] : 0.f;
        pre += below;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const int pos = tid * IPT + k;
            if (pos < n && !(pre < top_p || pos < beam)) qv[idx_b[pos]] = -1.f;
            pre += loc[k];
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += NT) {
        const float me = qv[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += (qv[j] > me) || (qv[j] == me && j < i);
        if (r < beam) picks[r] = i;
    }
    __syncthreads();
    if (tid < 64) {
        // log_softmax over the gathered (un-tempered) logits of the picks (beam.py:79): lane b owns pick b
        const int pi = tid < beam ? picks[tid] : -1;
        const float lv = pi >= 0 ? val_a[pi] : -INFINITY;
        // fewer positive-probability tokens than beams: a survivor at -inf (a threshold of -inf keeps them all) is a dead pick too
        const int n_live = __popcll(__ballot(lv > -INFINITY));
        if (tid == 0 && n_live < beam) atomicOr(err, DH_BEAM_ERR_TOO_FEW);
        const float mx = wave_max(lv);
        const float se = wave_sum(pi >= 0 ? expf(lv - mx) : 0.f);
        const float lse = logf(se);
        if (tid < beam) {
            pick_store(pick_idx, pick_val, (size_t)rc * beam + tid, pi >= 0 ? idx_a[pi] : 0, pi >= 0 ? (lv - mx) - lse : -INFINITY);
        }
    }
#undef s_cnt
#undef s_thr
}

template <int EPT, int NT, int WPE, bool PR, bool NU = false>
__global__ __launch_bounds__(NT, WPE) void beam_row_sample_fast_kernel(
    const float* __restrict__ logits, int ldl, int V, int rows_per_img, int beam, int top_k,
    float temperature, int unk, const float* __restrict__ noise, uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step,
    int32_t* __restrict__ pick_idx, float* __restrict__ pick_val, int32_t* __restrict__ err, const int32_t* __restrict__ first_pos,
    float top_p) {
    __shared__ uint32_t lmax[NT];
    __shared__ int hist[4 * 256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k, s_cnt, wtot[4];
    __shared__ __attribute__((aligned(16))) int idx_a[CAP], idx_b[CAP];
    __shared__ __attribute__((aligned(16))) float val_a[CAP], val_b[CAP], qv[CAP];
    __shared__ float red[NT];
    __shared__ int picks[DH_BEAM_MAX_BEAMS];
    __shared__ uint32_t s_thr;

    const int rc = blockIdx.x, tid = threadIdx.x;
    if constexpr (PR) { if (prompt_row_idle(first_pos, rc, rows_per_img, step)) return; }
    const float* row = logits + (size_t)rc * ldl;
    float v[EPT];
    uint32_t best = 0u;                          // key 0 < key of every real float
    // buffer loads: one shared per-lane offset + scalar strides, hardware bounds check (reads past V
    // return 0 and are ignored below) -> ~1 VGPR per element instead of an address pair + predicate
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, V * 4, 0x00020000);
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, tid * 4, e * NT * 4, 0));
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * NT;
        if (i < V) best = max(best, f2key(v[e]));
    }
    lmax[tid] = best;
    if (tid == 0) { s_prefix = 0u; s_k = top_k; s_cnt = 0; s_thr = 0u; }
    // k-th largest of the 512 thread maxima (one key per thread: cheap LDS radix select)
    uint32_t mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        if ((best & mask) == prefix) atomicAdd(&hist[(best >> shift) & 255u], 1);
        __syncthreads();
        radix_pick_digit(hist, 1, shift, prefix, &s_prefix, &s_k, wtot);
        mask |= 0xFFu << shift;
    }
    const uint32_t bound = s_prefix;             // <= key of the row's k-th largest value
    // compact every value >= bound
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * NT;
        if (i < V && f2key(v[e]) >= bound) {
            const int p = atomicAdd(&s_cnt, 1);
            if (p < CAP) { idx_a[p] = i; val_a[p] = v[e]; }
        }
    }
    __syncthreads();
    if (s_cnt > CAP) radix_row_candidates<NT>(row, V, top_k, hist, &s_prefix, &s_k, &s_cnt, wtot, idx_a, val_a);
    const RowLds L{idx_a, idx_b, val_a, val_b, qv, red, picks, &s_cnt, &s_thr};
    row_tail<NT, NU>(L, rc, ldl, rows_per_img, beam, top_k, temperature, unk, noise, seed, seed_ptr, img0, step, pick_idx, pick_val, err, top_p);
}

// ---- candidate draw of one image (beam_select_kernel) -----------------------------------------------------------------------
struct SelectParams {
    const int32_t* pick_idx; const float* pick_val;
    int32_t* tokens; int tok_ld; float* vals; uint8_t* ended; int32_t* src; int src_ld;
    int32_t* parent; int32_t* hparent; uint8_t* done; int32_t* end_step;
    int beam, first, first_sets_ended, write_pos, t, step_index, eos, img0;
    float temperature; const float* noise; uint64_t seed; const uint64_t* seed_ptr;
    const int32_t* first_pos = nullptr;                 // dh_beam_select_prompted: [n_img] prompt lengths, `first` is then per image
    float* keys = nullptr;                              // dh_beam_select_best_norm: [rows] the kept candidates' keys (score * len_w[L])
    const float* len_w = nullptr;                       //   [tok_ld + 1] weights by generated length, len_w[0] = 1
    int first_col = 0;                                  //   dense: the first generated column (prompted: first_pos[img])
    int32_t* pool_tokens = nullptr;                     // dh_beam_select_pool: [n_img, beam, tok_ld] the finished hypotheses, slot 0 the best
    float* pool_keys = nullptr; float* pool_vals = nullptr;     //   [n_img, beam] their keys (descending) and raw scores
    int32_t* pool_len = nullptr; int32_t* pool_n = nullptr;     //   [n_img, beam] their lengths (<eos> included), [n_img] entries held
    int stop_when_full = 0;                             //   early_stopping=True: done as soon as the pool is full
    int n_groups = 1;                                   // dh_beam_select_groups: slots g * (beam / n_groups) .. are group g
    float diversity = 0.f;                              //   what every earlier group's use of a token at this position costs its key
};

// LDS scratch of one image's candidate draw, carved by the caller (beam_select_kernel's own arrays)
struct SelLds {
    int32_t* stage;                                     // [beam][tok_ld] tokens, then [beam][t] ancestors
    int* ctok; int* cpar; int* keep; float* cval; float* q; uint8_t* cend; int* s_n;
    int32_t* pki = nullptr; float* pkv = nullptr;       // optional [beam * beam]: the image's picks, brought in with the first round trip
    int* ord = nullptr; int* offer = nullptr;           // dh_beam_select_pool: [2 * beam] candidates by rank, [beam] the <eos> candidates offered
    float* pen = nullptr; int* said = nullptr;          // dh_beam_select_groups: [beam * beam] penalised keys, [2 * beam + 1] tokens taken + group starts
};

// The candidate draw + in-place rewrite of one image's beam state, executed by ONE wave (lane = 0..63); LDS hand-overs are
// wave-local (wave_lds_sync).  MB = the largest beam
// count the instantiation takes (register arrays of the beams' flags / scores): 16 for the usual settings, 64 for beam_size > 16.
// PR (dh_beam_select_prompted): the image's phase comes from p.first_pos[img] against p.step_index instead of the launch-wide p.first
// (see prompt_row_idle); its first step reads the picks of its logical row img * beam, where the prompted samplers leave them.
// DT (dh_beam_select_best): no draw -- the `beam` candidates with the largest score stay, equal scores to the lower candidate index,
// -inf last; hparent is the real parent row.  Neither noise nor temperature is read.
// LN (dh_beam_select_best_norm, with DT): the rank runs on key = score * len_w[L] in place of the score -- ONE fp32 multiply; L, the
// columns the search has written to a live candidate, is write_pos + 1 - (the image's first generated column), the same for every live
// candidate of the image, so len_w[L] is one wave-uniform load.  An ended beam's candidate keeps the key it was kept with (p.keys,
// loaded with vals and ended); q holds the keys, the kept ones go to p.keys, and p.vals keeps the raw scores.
// PL (dh_beam_select_pool, with DT and LN): what follows the candidate list of an image under early_stopping -- the rank, the walk over
// it, the pool insertion, the rewrite and the done rule.  n candidates stand in ctok / cval / cpar with their keys in q.
//   rank   : ord[r] = the candidate of rank r for r < min(n, 2 * beam): larger key first, equal keys to the lower candidate index (a first
//            step keeps pick order).  At most `beam` candidates are <eos> (one per live row), so 2 * beam ranks hold `beam` others.
//   walk   : 64 ranks per round, a ballot each for "takes a live slot" (not <eos>, key > -inf) and "offered" (<eos>, rank < beam, key >
//            -inf); a candidate's slot / offer number is the count of set bits below its lane: rank order, no atomics.
//   rewrite: slot b < taken as the LN select writes a kept candidate, with ended = 0; the others are dead slots -- their own row with
//            token 0, vals = keys = -inf, ended = 1, parent = hparent = src[.., t] = themselves (at a first step: the image's base row).
//   pool   : lane j holds entry j's key / score / length in registers; an offer goes behind every entry with key >= its own (ballot),
//            the entries below move one down (register shuffles; the token rows from the bottom up, each lane its own columns: plain
//            vector stores in a fixed order) and entry `beam` falls off -- a full pool is entered only strictly above its worst key.
//   done   : the pool is full, and early_stopping is True or the pool's worst key >= live slot 0's (-inf for a dead slot).
template <int MB>
__device__ __forceinline__ void beam_pool_tail(const SelectParams& p, const int img, const int lane, const SelLds& L, const int n,
                                               const int first, const bool pre) {
    const int B = p.beam, base = img * B;
    int* ctok = L.ctok; int* cpar = L.cpar; int* keep = L.keep; float* cval = L.cval; float* q = L.q;
    int* ord = L.ord; int* offer = L.offer;
    // the pool's scalars, in flight while the rank runs
    int n_pool = min(max(p.pool_n[img], 0), B);
    float pk = -INFINITY, pv = -INFINITY;
    int pl = 0;
    if (lane < B) { pk = p.pool_keys[base + lane]; pv = p.pool_vals[base + lane]; pl = p.pool_len[base + lane]; }
    const int nr = min(n, 2 * B);
    for (int r = lane; r < nr; r += 64) ord[r] = r;        // (every entry valid whatever the keys are, as `keep` in the other selects)
    wave_lds_sync();
    if (!first) {
        for (int c = lane; c < n; c += 64) {
            const float me = q[c];
            int r = 0;
            for (int j = 0; j < n; ++j) r += (q[j] > me) || (q[j] == me && j < c);
            if (r < nr) ord[r] = c;
        }
        wave_lds_sync();
    }
    int taken = 0, n_off = 0;                             // (wave-uniform)
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r0 = 0; r0 < nr; r0 += 64) {
        const int r = r0 + lane;
        bool live = false, off = false;
        int c = 0;
        if (r < nr) {
            c = ord[r];
            const bool fin = q[c] > -INFINITY, eos = ctok[c] == p.eos;
            live = fin && !eos;
            off = fin && eos && r < B;
        }
        const unsigned long long lb = __ballot(live), ob = __ballot(off);
        if (live) { const int s = taken + __popcll(lb & below); if (s < B) keep[s] = c; }
        if (off) offer[n_off + __popcll(ob & below)] = c;  // (only ranks < beam are offered: at most `beam` entries)
        taken += __popcll(lb); n_off += __popcll(ob);
    }
    taken = min(taken, B);
    int32_t* tokbuf = L.stage;
    int32_t* srcbuf = L.stage + (size_t)B * p.tok_ld;
    if (!pre) {
        for (int i = lane; i < B * p.tok_ld; i += 64) tokbuf[i] = p.tokens[(size_t)base * p.tok_ld + i];
        if (p.src)
            for (int b = 0; b < B; ++b)
                for (int j = lane; j < p.t; j += 64) srcbuf[b * p.t + j] = p.src[(size_t)(base + b) * p.src_ld + j];
    }
    wave_lds_sync();
    for (int b = 0; b < B; ++b) {
        const bool dead = b >= taken;
        const int c = dead ? 0 : keep[b];
        // (a first step: only the image's base row has history behind it -- LSTM state, KV cache --, so a dead slot points there, like
        //  the rows of a forced image; its token row is the base row's, which holds the same prefix)
        const int par = dead ? (first ? 0 : b) : cpar[c], tok = dead ? 0 : ctok[c];
        for (int i = lane; i < p.tok_ld; i += 64)
            p.tokens[(size_t)(base + b) * p.tok_ld + i] = (i == p.write_pos) ? tok : tokbuf[par * p.tok_ld + i];
        if (p.src) {
            for (int j = lane; j < p.t; j += 64) p.src[(size_t)(base + b) * p.src_ld + j] = srcbuf[par * p.t + j];
            if (lane == 0) p.src[(size_t)(base + b) * p.src_ld + p.t] = base + par;
        }
        if (lane == 0) {
            p.vals[base + b] = dead ? -INFINITY : cval[c];
            p.keys[base + b] = dead ? -INFINITY : q[c];
            p.ended[base + b] = (uint8_t)dead;
            p.parent[base + b] = base + par;
            p.hparent[base + b] = base + par;
        }
    }
    int32_t* pt = p.pool_tokens + (size_t)base * p.tok_ld;
    for (int o = 0; o < n_off; ++o) {
        const int c = offer[o], par = cpar[c];
        const float ok = q[c];
        const int at = __popcll(__ballot(lane < n_pool && pk >= ok));
        if (at >= B) continue;                            // (wave-uniform) a full pool whose worst key is >= this one
        for (int j = min(n_pool, B - 1); j > at; --j)
            for (int i = lane; i < p.tok_ld; i += 64) pt[(size_t)j * p.tok_ld + i] = pt[(size_t)(j - 1) * p.tok_ld + i];
        for (int i = lane; i < p.tok_ld; i += 64) pt[(size_t)at * p.tok_ld + i] = (i == p.write_pos) ? p.eos : tokbuf[par * p.tok_ld + i];
        const float uk = __shfl_up(pk, 1), uv = __shfl_up(pv, 1);
        const int ul = __shfl_up(pl, 1);
        if (lane == at) { pk = ok; pv = cval[c]; pl = p.write_pos + 1; }
        else if (lane > at) { pk = uk; pv = uv; pl = ul; }
        n_pool = min(n_pool + 1, B);
    }
    if (n_off > 0) {
        if (lane < B) { p.pool_keys[base + lane] = pk; p.pool_vals[base + lane] = pv; p.pool_len[base + lane] = pl; }
        if (lane == 0) p.pool_n[img] = n_pool;
    }
    if (n_pool == B) {                                    // (wave-uniform)
        const float worst = __shfl(pk, B - 1);
        const float top = taken > 0 ? q[keep[0]] : -INFINITY;
        if (lane == 0 && (p.stop_when_full || worst >= top)) { p.done[img] = 1; p.end_step[img] = p.step_index; }
    }
}

// GR (dh_beam_select_groups, with DT and LN): the rank of an image whose `beam` slots are p.n_groups groups of Bg = beam / n_groups --
// slots g * Bg .. g * Bg + Bg - 1 are group g from the first step to the last.  n candidates stand in ctok / cval / cpar with their
// keys in q; the candidates of group g are those whose parent slot lies in it (one contiguous run: the list is in parent order), at a
// first step -- one source row -- all of them.  The groups are ranked one after the other, g = 0 first:
//   said   : the tokens the kept candidates of the groups before g took at this position, in slot order (a kept candidate that is an
//            ended beam's filler, or whose key is not > -inf, adds nothing).
//   pen    : a candidate of a live row with a finite key gets q - diversity * (times its token stands in `said`) -- the product and the
//            difference rounded one by one (no FMA) --, every other pen = q; NaN ranks as -inf.
//   rank   : the Bg largest pen of the group go to slots g * Bg + rank, equal pen to the lower candidate index.  A slot is a rank and
//            `said` is appended through a ballot in slot order: no atomics.
// Only `keep` comes out of it: cval and q are not touched, so what the common rewrite stores is not penalised.
__device__ __forceinline__ void beam_group_tail(const SelectParams& p, const int lane, const SelLds& L, const int n, const int first) {
    const int B = p.beam, G = p.n_groups, Bg = B / G;
    const int* ctok = L.ctok; const int* cpar = L.cpar; int* keep = L.keep; const float* q = L.q;
    float* pen = L.pen; int* said = L.said; int* gstart = L.said + B;
    // a row that had ended stands in the list with ONE candidate, a live row with `beam` >= 2 of them (n_groups > 1; with one group
    // nothing is ever penalised or counted): a candidate whose neighbours both have other parents is an ended beam's filler
    auto filler = [&](int c) { return !first && (c == 0 || cpar[c - 1] != cpar[c]) && (c + 1 == n || cpar[c + 1] != cpar[c]); };
    if (!first) {
        for (int c = lane; c < n; c += 64) {
            const int g = cpar[c] / Bg;
            if (c == 0 || cpar[c - 1] / Bg != g) gstart[g] = c;
        }
        if (lane == 0) gstart[G] = n;
        wave_lds_sync();
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int n_said = 0;                                       // (wave-uniform)
    for (int g = 0; g < G; ++g) {
        const int lo = first ? 0 : gstart[g], hi = first ? n : gstart[g + 1];
        for (int c = lo + lane; c < hi; c += 64) {
            const float k = q[c];
            float v = k;
            if (fabsf(k) < INFINITY && !filler(c)) {
                const int tok = ctok[c];
                int cnt = 0;
                for (int s = 0; s < n_said; ++s) cnt += said[s] == tok;
                v = __fsub_rn(k, __fmul_rn(p.diversity, (float)cnt));
            }
            pen[c] = v != v ? -INFINITY : v;
        }
        // (every slot valid whatever the keys are, as in the other selects: a group holds at least Bg candidates)
        for (int r = lane; r < Bg; r += 64) keep[g * Bg + r] = lo + min(r, hi - lo - 1);
        wave_lds_sync();
        for (int c = lo + lane; c < hi; c += 64) {
            const float me = pen[c];
            int r = 0;
            for (int j = lo; j < hi; ++j) r += (pen[j] > me) || (pen[j] == me && j < c);
            if (r < Bg) keep[g * Bg + r] = c;
        }
        wave_lds_sync();
        bool adds = false;
        int tok = 0;
        if (lane < Bg) {
            const int c = keep[g * Bg + lane];
            tok = ctok[c];
            adds = q[c] > -INFINITY && !filler(c);
        }
        const unsigned long long ab = __ballot(adds);
        if (adds) said[n_said + __popcll(ab & below)] = tok;      // (at most Bg per group: never more than `beam` entries)
        n_said += __popcll(ab);
        wave_lds_sync();
    }
}

template <int MB, bool PR = false, bool DT = false, bool LN = false, bool PL = false, bool GR = false>
__device__ __forceinline__ void beam_select_image(const SelectParams& p, const int img, const int lane, const SelLds& L) {
    static_assert(DT || !LN, "the length weights rank the deterministic select only");
    static_assert(LN || !PL, "the pool ranks by key");
    static_assert((DT && LN && !PL) || !GR, "the groups rank the keys of the deterministic select, without a pool");
    int32_t* stage = L.stage;
    int* ctok = L.ctok; int* cpar = L.cpar; int* keep = L.keep; float* cval = L.cval; float* q = L.q; uint8_t* cend = L.cend;
#define s_n (*L.s_n)
    const int B = p.beam, base = img * B;
    int first = p.first;
    int first_col = p.first_col;
    if constexpr (PR) {
        const int fp = p.first_pos[img];
        first_col = fp;
        if (p.step_index < fp) {
            // forced: the token column keeps the prompt's token, scores / ended / done stay 0, nothing is drawn.  Every beam row keeps
            // pointing at the image's base row -- the one row with real history behind it -- for the KV cache and the LSTM state
            for (int b = lane; b < B; b += 64) {
                p.parent[base + b] = base; p.hparent[base + b] = base;
                if (p.src) p.src[(size_t)(base + b) * p.src_ld + p.t] = base;
            }
            return;
        }
        first = p.step_index == fp;
    }
    const size_t pk_first = PR ? (size_t)base * B : (size_t)img * B;
    // Stand-alone kernel (L.pki set): EVERYTHING the image needs -- its token rows, ancestor rows and all its picks -- is requested
    // up front by LDS-DMA, next to the loads of done / ended / vals: ONE memory round trip instead of four dependent ones (done ->
    // ended -> picks -> token rows), which were most of this 8 us kernel.
    const bool pre = L.pki != nullptr;
    int32_t* const tokbuf0 = stage;
    int32_t* const srcbuf0 = stage + (size_t)B * p.tok_ld;
    if (pre) {
        for (int i = lane; i < B * p.tok_ld; i += 64) dh_lds_dma4(p.tokens + (size_t)base * p.tok_ld + i, tokbuf0 + (i - lane));
        if (p.src)
            for (int b = 0; b < B; ++b)
                for (int j = lane; j < p.t; j += 64) dh_lds_dma4(p.src + (size_t)(base + b) * p.src_ld + j, srcbuf0 + b * p.t + (j - lane));
        const int npk = first ? B : B * B;
        const size_t pk0 = first ? pk_first : (size_t)base * B;
        for (int i = lane; i < npk; i += 64) {
            dh_lds_dma4(p.pick_idx + pk0 + i, L.pki + (i - lane));
            dh_lds_dma4(p.pick_val + pk0 + i, L.pkv + (i - lane));
        }
    }
    const uint8_t is_done = p.done[img];
    uint8_t was_ended[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) was_ended[b] = p.ended[base + min(b, B - 1)];   // one round trip for all
    float val_b[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) val_b[b] = p.vals[base + min(b, B - 1)];
    float key_b[LN ? MB : 1];
    float w_len = 1.f;
    if constexpr (LN) {
#pragma unroll
        for (int b = 0; b < MB; ++b) key_b[b] = p.keys[base + min(b, B - 1)];
        w_len = p.len_w[min(max(p.write_pos + 1 - first_col, 0), p.tok_ld)];      // (image-uniform; the table has tok_ld + 1 entries)
    }
    if (pre) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); wave_lds_sync(); }
    if (is_done) return;

    // candidate list in the reference's order: beam b contributes 1 candidate if it has ended, else B.
    // Every lane derives the (short) offset table itself; candidates are then filled in parallel.
    if (first) {
        for (int j = lane; j < B; j += 64) {
            const int tok = pre ? L.pki[j] : p.pick_idx[pk_first + j];
            ctok[j] = tok; cval[j] = pre ? L.pkv[j] : p.pick_val[pk_first + j]; cpar[j] = 0;
            cend[j] = (uint8_t)(p.first_sets_ended && tok == p.eos);
            if constexpr (LN) q[j] = cval[j] * w_len;
            keep[j] = j;
        }
        if (lane == 0) s_n = B;
    } else {
        int off[MB + 1];
        off[0] = 0;
#pragma unroll
        for (int b = 0; b < MB; ++b)
            off[b + 1] = off[b] + (b < B ? (was_ended[b] ? 1 : B) : 0);
        const int total = off[B];
        for (int c = lane; c < total; c += 64) {
            int b = 0;
#pragma unroll
            for (int k = 1; k < MB; ++k) b += (k < B && c >= off[k]);
            const int j = c - off[b];
            bool was = false; float vb = 0.f;             // (static register indexing: b is a run-time value)
            [[maybe_unused]] float kb = 0.f;
#pragma unroll
            for (int k = 0; k < MB; ++k) if (k == b) { was = was_ended[k] != 0; vb = val_b[k]; if constexpr (LN) kb = key_b[k]; }
            const int tok = was ? 0 : (pre ? L.pki[b * B + j] : p.pick_idx[(size_t)(base + b) * B + j]);
            ctok[c] = tok;
            cval[c] = vb + (was ? 0.f : (pre ? L.pkv[b * B + j] : p.pick_val[(size_t)(base + b) * B + j]));
            if constexpr (LN) q[c] = was ? kb : cval[c] * w_len;      // an ended beam's key is carried, never recomputed
            cpar[c] = b;
            cend[c] = (uint8_t)(was || tok == p.eos);
        }
        if (lane == 0) s_n = total;
    }
    wave_lds_sync();
    const int n = s_n;
    if constexpr (PL) {
        beam_pool_tail<MB>(p, img, lane, L, n, first, pre);
        return;
    }
    if constexpr (GR) {
        beam_group_tail(p, lane, L, n, first);
    } else if constexpr (DT) {
        if (!first) {
            for (int j = lane; j < B; j += 64) keep[j] = min(j, n - 1);
            wave_lds_sync();
            const float* rank = LN ? q : cval;
            for (int c = lane; c < n; c += 64) {
                const float me = rank[c];
                int r = 0;
                for (int j = 0; j < n; ++j) r += (rank[j] > me) || (rank[j] == me && j < c);
                if (r < B) keep[r] = c;
            }
        }
    } else if (!first) {
        // draw `beam` candidates without replacement from softmax(cand_val / T)
        float m = -INFINITY;
        for (int c = lane; c < n; c += 64) m = fmaxf(m, cval[c] / p.temperature);
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < n; c += 64) { const float e = expf(cval[c] / p.temperature - m); q[c] = e; s += e; }
        s = wave_sum(s);
        for (int c = lane; c < n; c += 64) {
            const float nz = p.noise ? p.noise[(size_t)img * B * B + c]
                                     : philox_exp1(p.seed ^ (p.seed_ptr ? *p.seed_ptr : 0ull), (uint32_t)(p.img0 + img), (uint32_t)p.step_index, 1u, 0u, (uint32_t)c);
            q[c] = (q[c] / s) / nz;
        }
        // (every slot valid whatever the scores are: with a NaN among them no rank below comes out right, and the rewrite loop must
        //  not index with what the LDS held before)
        for (int j = lane; j < B; j += 64) keep[j] = min(j, n - 1);
        wave_lds_sync();
        for (int c = lane; c < n; c += 64) {
            const float me = q[c];
            int r = 0;
            for (int j = 0; j < n; ++j) r += (q[j] > me) || (q[j] == me && j < c);
            if (r < B) keep[r] = c;
        }
    }
    // stage the image's token rows and ancestor rows, then rewrite them in place
    int32_t* tokbuf = stage;
    int32_t* srcbuf = stage + (size_t)B * p.tok_ld;
    if (!pre) {
        for (int i = lane; i < B * p.tok_ld; i += 64) tokbuf[i] = p.tokens[(size_t)base * p.tok_ld + i];
        if (p.src)
            for (int b = 0; b < B; ++b)
                for (int j = lane; j < p.t; j += 64) srcbuf[b * p.t + j] = p.src[(size_t)(base + b) * p.src_ld + j];
    }
    wave_lds_sync();
    int all_ended = 1;
    for (int b = 0; b < B; ++b) {
        const int c = keep[b], par = cpar[c];
        for (int i = lane; i < p.tok_ld; i += 64)
            p.tokens[(size_t)(base + b) * p.tok_ld + i] = (i == p.write_pos) ? ctok[c] : tokbuf[par * p.tok_ld + i];
        if (p.src) {
            for (int j = lane; j < p.t; j += 64) p.src[(size_t)(base + b) * p.src_ld + j] = srcbuf[par * p.t + j];
            if (lane == 0) p.src[(size_t)(base + b) * p.src_ld + p.t] = base + par;
        }
        if (lane == 0) {
            p.vals[base + b] = cval[c];
            if constexpr (LN) p.keys[base + b] = q[c];
            p.ended[base + b] = cend[c];
            p.parent[base + b] = base + par;
            p.hparent[base + b] = DT ? base + par : base + c / B;        // rnn_models.py:135-137: dense B*B layout index
        }
        all_ended &= cend[c];
    }
    // the reference only tests all_ended() inside the token loop (rnn_models.py:131), never after the first draw
    if (lane == 0 && all_ended && !first) { p.done[img] = 1; p.end_step[img] = p.step_index; }
#undef s_n
}

// ---- group-max guided variant -----------------------------------------------------------------------------
// The vocabulary GEMM (dh_vocab_logits) leaves, next to the logits, the maximum of every group of `gcols`
// consecutive columns of each row.  The k-th largest GROUP maximum is a lower bound of the row's k-th largest
// value (k groups hold a value >= it), and only groups whose maximum reaches that bound can contain one of the
// top-k values: about top_k of the ~570 groups.  So this kernel reads ~9 % of the row instead of all of it.
template <int NT, bool PR, bool NU = false>
__global__ __launch_bounds__(NT) void beam_row_sample_groups_kernel(
    const float* __restrict__ logits, int ldl, int V, const float* __restrict__ gmax, int gm_ld, int n_groups,
    int gcols, int rows_per_img, int beam, int top_k, float temperature, int unk, const float* __restrict__ noise,
    uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* __restrict__ pick_idx, float* __restrict__ pick_val,
    int32_t* __restrict__ err, const int32_t* __restrict__ first_pos, float top_p) {
    constexpr int MAXG = 1024, GPT = MAXG / NT;       // group keys per thread, kept in registers
    __shared__ int glist[MAXG];
    __shared__ int hist[4][256];
    __shared__ uint32_t s_prefix, s_thr;
    __shared__ int s_k, s_cnt, s_ng, wtot[4];
    __shared__ __attribute__((aligned(16))) int32_t pool[5 * CAP];       // the five candidate buffers
    int* const idx_a = pool; int* const idx_b = pool + CAP;
    float* const val_a = reinterpret_cast<float*>(pool + 2 * CAP); float* const val_b = reinterpret_cast<float*>(pool + 3 * CAP);
    float* const qv = reinterpret_cast<float*>(pool + 4 * CAP);
    __shared__ float red[NT];
    __shared__ int picks[DH_BEAM_MAX_BEAMS];
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PR) { if (prompt_row_idle(first_pos, rc, rows_per_img, step)) return; }
    const float* row = logits + (size_t)rc * ldl;
    uint32_t gk[GPT];
#pragma unroll
    for (int e = 0; e < GPT; ++e) {
        // unconditional loads at a clamped index (one memory round trip for all of them, not one per conditional load)
        const int g = tid + e * NT;
        const uint32_t k = f2key(gmax[(size_t)rc * gm_ld + min(g, n_groups - 1)]);
        gk[e] = g < n_groups ? k : 0u;                                        // key 0 < key of every real float
    }
    for (int i = tid; i < 512; i += NT) (&hist[0][0])[i] = 0;
    if (tid == 0) { s_prefix = 0u; s_k = min(top_k, n_groups); s_cnt = 0; s_ng = 0; s_thr = 0u; }
    __syncthreads();
    // Lower edge of the 16-bit key bucket (sign, exponent, 7 mantissa bits) that holds the k-th largest group maximum:
    // at least k groups -- hence at least k logits -- are >= it, and only a handful of extra groups share the bucket.
    // Two radix passes instead of the four an exact k-th largest needs.
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t prefix = s_prefix, mask = pass == 0 ? 0u : 0xFF000000u;
#pragma unroll
        for (int e = 0; e < GPT; ++e)
            if (tid + e * NT < n_groups && (gk[e] & mask) == prefix) atomicAdd(&hist[pass][(gk[e] >> shift) & 255u], 1);
        __syncthreads();
        radix_pick_digit(hist[pass], 1, shift, prefix, &s_prefix, &s_k, wtot);
    }
    const uint32_t bound = s_prefix;                 // <= the row's k-th largest logit (as a key)
#pragma unroll
    for (int e = 0; e < GPT; ++e)
        if (tid + e * NT < n_groups && gk[e] >= bound) glist[atomicAdd(&s_ng, 1)] = tid + e * NT;
    __syncthreads();
    const int ng = s_ng;
    // one wave per selected group (coalesced 256-B reads), all of a wave's groups requested before the first is used
    constexpr int NWV = NT / 64, UN = 16;     // 64 groups in one round of loads (a row selects ~55)
    for (int q0 = wave; q0 < ng; q0 += NWV * UN) {
        float v[UN]; int ci[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int q = q0 + u * NWV;
            ci[u] = q < ng ? glist[min(q, ng - 1)] * gcols + lane : V;
            v[u] = row[min(ci[u], V - 1)];                  // unconditional (clamped) loads: all in flight together
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (lane < gcols && ci[u] < V && f2key(v[u]) >= bound) {
                const int pp = atomicAdd(&s_cnt, 1);
                if (pp < CAP) { idx_a[pp] = ci[u]; val_a[pp] = v[u]; }
            }
    }
    __syncthreads();
    if (s_cnt > CAP) radix_row_candidates<NT>(row, V, top_k, &hist[0][0], &s_prefix, &s_k, &s_cnt, wtot, idx_a, val_a);
    const RowLds L{idx_a, idx_b, val_a, val_b, qv, red, picks, &s_cnt, &s_thr};
    row_tail<NT, NU>(L, rc, ldl, rows_per_img, beam, top_k, temperature, unk, noise, seed, seed_ptr, img0, step, pick_idx, pick_val, err, top_p);
}

// The launches of the three row-sampler entry points and of their *_prompted twins (PR: with first_pos, see prompt_row_idle)
template <bool PR, bool NU = false>
static int row_sample_groups_launch(const float* logits, int ldl, int V, const float* group_max, int gm_ld,
                                    int n_groups, int group_cols, int rows, int rows_per_img, int beam,
                                    int top_k, float temperature, int unk_index, const float* noise,
                                    uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                    int32_t* pick_idx, float* pick_val, int32_t* err, void* stream, float top_p = 1.f) {
    DH_REQUIRE(logits && group_max && pick_idx && pick_val && err && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V);
    DH_REQUIRE(beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && beam <= top_k && top_k <= V && temperature > 0.f);
    DH_REQUIRE(n_groups > 0 && n_groups <= 1024 && top_k <= n_groups && gm_ld >= n_groups && group_cols > 0 && group_cols <= 64 &&
               (long long)n_groups * group_cols >= V);
    DH_REQUIRE(!PR || (first_pos && rows_per_img == beam && rows % beam == 0));
    DhProfScope prof(NU ? "dh_beam_row_sample_nucleus" : "dh_beam_row_sample", 0.0, 0.0, stream);
    hipLaunchKernelGGL((beam_row_sample_groups_kernel<256, PR, NU>), dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V,
                       group_max, gm_ld, n_groups, group_cols, rows_per_img, beam, top_k, temperature, unk_index, noise,
                       seed, seed_ptr, img0, step, pick_idx, pick_val, err, first_pos, top_p);
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_row_sample_groups(const float* logits, int ldl, int V, const float* group_max, int gm_ld,
                                         int n_groups, int group_cols, int rows, int rows_per_img, int beam,
                                         int top_k, float temperature, int unk_index, const float* noise,
                                         uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* pick_idx, float* pick_val,
                                         int32_t* err, void* stream) {
    return row_sample_groups_launch<false>(logits, ldl, V, group_max, gm_ld, n_groups, group_cols, rows, rows_per_img, beam, top_k, temperature,
                                           unk_index, noise, seed, seed_ptr, img0, step, nullptr, pick_idx, pick_val, err, stream);
}

extern "C" int dh_beam_row_sample_groups_prompted(const float* logits, int ldl, int V, const float* group_max, int gm_ld,
                                                  int n_groups, int group_cols, int rows, int rows_per_img, int beam,
                                                  int top_k, float temperature, int unk_index, const float* noise,
                                                  uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                                  int32_t* pick_idx, float* pick_val, int32_t* err, void* stream) {
    return row_sample_groups_launch<true>(logits, ldl, V, group_max, gm_ld, n_groups, group_cols, rows, rows_per_img, beam, top_k, temperature,
                                          unk_index, noise, seed, seed_ptr, img0, step, first_pos, pick_idx, pick_val, err, stream);
}

// exact: the general kernel only (4-pass radix select over the whole row; any top_k, any V; a row with more survivors than
// DH_BEAM_MAX_SURVIVORS is drawn over the row itself instead of flagging DH_BEAM_ERR_OVERFLOW): the fall-back the host takes when a batch
// flagged that overflow in the pre-filtered kernels.
template <bool PR, bool NU = false>
static int row_sample_launch(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                             int top_k, float temperature, int unk_index, const float* noise,
                             uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos, int32_t* pick_idx,
                             float* pick_val, int32_t* err, bool exact, void* stream, float top_p = 1.f) {
    DH_REQUIRE(logits && pick_idx && pick_val && err && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V);
    DH_REQUIRE(beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && beam <= top_k && top_k <= V && temperature > 0.f);
    DH_REQUIRE(!PR || (first_pos && rows_per_img == beam && rows % beam == 0));
    DhProfScope prof(NU ? "dh_beam_row_sample_nucleus" : "dh_beam_row_sample", 0.0, 0.0, stream);
#define DH_FAST(EPT, NT, WPE) hipLaunchKernelGGL((beam_row_sample_fast_kernel<EPT, NT, WPE, PR, NU>), dim3(rows), dim3(NT), 0, \
        (hipStream_t)stream, logits, ldl, V, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, \
        step, pick_idx, pick_val, err, first_pos, top_p)
    if (!exact && top_k <= 256 && V <= 512 * 8) DH_FAST(8, 512, 4);
    else if (!exact && top_k <= 256 && V <= 1024 * 16) DH_FAST(16, 1024, 8);
    else if (!exact && top_k <= 256 && V <= 1024 * 36) DH_FAST(36, 1024, 8);
    else if (!exact && top_k <= 256 && V <= 1024 * 64) DH_FAST(64, 1024, 4);
    else
        hipLaunchKernelGGL((beam_row_sample_kernel<PR, NU>), dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V,
                           rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, step, pick_idx,
                           pick_val, err, first_pos, top_p);
#undef DH_FAST
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_row_sample(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                  int top_k, float temperature, int unk_index, const float* noise,
                                  uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* pick_idx, float* pick_val,
                                  int32_t* err, void* stream) {
    return row_sample_launch<false>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, step,
                                    nullptr, pick_idx, pick_val, err, false, stream);
}

extern "C" int dh_beam_row_sample_exact(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                        int top_k, float temperature, int unk_index, const float* noise,
                                        uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0, int step, int32_t* pick_idx, float* pick_val,
                                        int32_t* err, void* stream) {
    return row_sample_launch<false>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, step,
                                    nullptr, pick_idx, pick_val, err, true, stream);
}

extern "C" int dh_beam_row_sample_prompted(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                           int top_k, float temperature, int unk_index, const float* noise,
                                           uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                           int32_t* pick_idx, float* pick_val, int32_t* err, void* stream) {
    return row_sample_launch<true>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, step,
                                   first_pos, pick_idx, pick_val, err, false, stream);
}

extern "C" int dh_beam_row_sample_exact_prompted(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                                 int top_k, float temperature, int unk_index, const float* noise,
                                                 uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                                 int32_t* pick_idx, float* pick_val, int32_t* err, void* stream) {
    return row_sample_launch<true>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0, step,
                                   first_pos, pick_idx, pick_val, err, true, stream);
}

// Nucleus (top-p) row draw, every route through one entry point: the NU = true instantiations of the three kernels above.
// exact != 0: the general kernel; else group_max != NULL: the group-guided kernel; else the single-pass kernels by V as dh_beam_row_sample
// picks them.  first_pos != NULL: the prompted phases (prompt_row_idle).  top_p outside (0, 1) is a bad argument: 1 is the callers'
// "no nucleus", which is the other entry points' business.
extern "C" int dh_beam_row_sample_nucleus(const float* logits, int ldl, int V, const float* group_max, int gm_ld, int n_groups,
                                          int group_cols, int rows, int rows_per_img, int beam, int top_k, float top_p,
                                          float temperature, int unk_index, const float* noise, uint64_t seed, const uint64_t* seed_ptr,
                                          int img0, int step, const int32_t* first_pos, int exact, int32_t* pick_idx, float* pick_val,
                                          int32_t* err, void* stream) {
    DH_REQUIRE(top_p > 0.f && top_p < 1.f);
    if (group_max && !exact) {
        if (first_pos)
            return row_sample_groups_launch<true, true>(logits, ldl, V, group_max, gm_ld, n_groups, group_cols, rows, rows_per_img, beam, top_k,
                                                        temperature, unk_index, noise, seed, seed_ptr, img0, step, first_pos, pick_idx, pick_val,
                                                        err, stream, top_p);
        return row_sample_groups_launch<false, true>(logits, ldl, V, group_max, gm_ld, n_groups, group_cols, rows, rows_per_img, beam, top_k,
                                                     temperature, unk_index, noise, seed, seed_ptr, img0, step, nullptr, pick_idx, pick_val, err,
                                                     stream, top_p);
    }
    if (first_pos)
        return row_sample_launch<true, true>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0,
                                             step, first_pos, pick_idx, pick_val, err, exact != 0, stream, top_p);
    return row_sample_launch<false, true>(logits, ldl, V, rows, rows_per_img, beam, top_k, temperature, unk_index, noise, seed, seed_ptr, img0,
                                          step, nullptr, pick_idx, pick_val, err, exact != 0, stream, top_p);
}

// ---- history-dependent logit edits (no_repeat_ngram_size, repetition_penalty) in front of the row draw ---------------------------
// One workgroup per logits row; the row's own history h[0 .. pos) is columns < pos of its token row (r * tok_row_mult: the dense
// first step has one logits row per image and the image's tokens at row img * beam).  Ids outside [0, V) take part in the n-gram
// comparison as they are and are never a column.  Three phases, a workgroup barrier between them:
//   1. penalty != 1: every history position READS its column (into LDS), barrier, every position WRITES x < 0 ? x * penalty : x / penalty of
//      the value it read.  All reads of the row precede all writes, so the positions of one token store the same word: each
//      distinct token is damped exactly once without a de-duplication pass (-inf stays -inf: -inf * penalty, penalty > 0).
//   2. ngram = n >= 1, pos >= n: position j in [0, pos - n] whose n - 1 tokens equal the row's last n - 1 bans h[j + n - 1]
//      (-inf; n == 1: every token of the history).  After the barrier, so a ban wins over the penalty's store to the same column.
//   3. group_max != NULL: every group that received a store is put on a list once (atomicExch on its flag), and after the barrier
//      (workgroup-scope release / acquire: the stores above are visible to the other waves of the CU) one wave per listed group reads
//      the group's columns back and stores their fp32 maximum.  CONVENTION: the maximum runs over the group's REAL columns (< V)
//      only.  dh_vocab_logits and dh_linear_f32xp do the same (`n < N` in their epilogues); dh_vocab_logits_wreg folds the written pad
//      columns of the last partial group in, which are copies of column V - 1 (pack_vocab_weights), so its word is the real columns'
//      maximum too -- until column V - 1 is edited: the pads then keep the old value, and a maximum over them would be one that no
//      column the sampler reads attains (its bound needs the k-th largest group maximum <= the k-th largest logit).  A group whose
//      real columns are all -inf gets -inf; groups without a store, groups past V among them, are not written.
// Forced / idle rows of a prompted launch leave before the first barrier (prompt_row_idle with step = pos).
__global__ __launch_bounds__(256) void beam_history_logits_kernel(
    float* logits, int ldl, int V, float* gmax, int gm_ld, int n_groups, int gcols, const int32_t* __restrict__ tokens, int tok_ld,
    int tok_row_mult, int pos, int rows_per_img, const int32_t* __restrict__ first_pos, int ngram, float penalty) {
    constexpr int NT = 256, PPT = DH_BEAM_MAX_HISTORY / NT, MAXG = 1024;
    __shared__ int hist[DH_BEAM_MAX_HISTORY];
    __shared__ float hval[DH_BEAM_MAX_HISTORY];      // the penalty's loaded logits, one per history position
    __shared__ int gflag[MAXG], glist[MAXG];
    __shared__ int s_ng;
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (first_pos && prompt_row_idle(first_pos, rc, rows_per_img, pos)) return;
    float* row = logits + (size_t)rc * ldl;
    const int32_t* h = tokens + (size_t)rc * tok_row_mult * tok_ld;
    const int L = pos;
    for (int i = tid; i < L; i += NT) hist[i] = h[i];
    if (gmax)
        for (int g = tid; g < n_groups; g += NT) gflag[g] = 0;
    if (tid == 0) s_ng = 0;
    __syncthreads();
    auto mark = [&](int t) {              // column t (< V <= n_groups * gcols) received a store
        if (gmax) {
            const int g = t / gcols;
            if (atomicExch(&gflag[g], 1) == 0) glist[atomicAdd(&s_ng, 1)] = g;
        }
    };
    if (penalty != 1.f) {
        int tk[PPT];
#pragma unroll
        for (int e = 0; e < PPT; ++e) {
            const int i = tid + e * NT;
            const int t = i < L ? hist[i] : -1;
            tk[e] = (t >= 0 && t < V) ? t : -1;
            hval[i] = tk[e] >= 0 ? row[tk[e]] : 0.f;
        }
        // Every load of the row has completed before any store to it: a thread parks what it loaded in LDS, which needs the loaded
        // word itself, before it reaches the barrier, and takes its own words back behind it.
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PPT; ++e)
            if (tk[e] >= 0) {
                const float x = hval[tid + e * NT];
                row[tk[e]] = x < 0.f ? x * penalty : __fdiv_rn(x, penalty);
                mark(tk[e]);
            }
        __syncthreads();
    }
    if (ngram >= 1 && L >= ngram) {
        const int m = ngram - 1, p0 = L - m;
        for (int j = tid; j + ngram <= L; j += NT) {
            bool eq = true;
            for (int k = 0; k < m && eq; ++k) eq = hist[j + k] == hist[p0 + k];
            const int t = hist[j + m];
            if (eq && t >= 0 && t < V) { row[t] = -INFINITY; mark(t); }
        }
    }
    if (gmax) {
        __threadfence_block();
        __syncthreads();
        const int ng = s_ng;
        for (int q = wave; q < ng; q += NT / 64) {
            const int g = glist[q], c = g * gcols + lane;
            float v = (lane < gcols && c < V) ? row[c] : -INFINITY;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
            if (lane == 0) gmax[(size_t)rc * gm_ld + g] = v;
        }
    }
}

extern "C" int dh_beam_history_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                                      const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                                      const int32_t* first_pos, int ngram, float penalty, void* stream) {
    DH_REQUIRE(logits && tokens && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V && tok_row_mult >= 1);
    DH_REQUIRE(pos >= 0 && pos <= tok_ld && pos <= DH_BEAM_MAX_HISTORY);
    DH_REQUIRE(ngram >= 0 && penalty > 0.f && penalty < INFINITY);            // (a NaN penalty fails both comparisons)
    DH_REQUIRE(ngram > 0 || penalty != 1.f);                                   // both controls off: the caller makes no launch
    DH_REQUIRE(!group_max || (n_groups > 0 && n_groups <= 1024 && gm_ld >= n_groups && group_cols > 0 && group_cols <= 64 &&
                              (long long)n_groups * group_cols >= V));         // dh_beam_row_sample_groups' contract
    DH_REQUIRE(!first_pos || rows % rows_per_img == 0);
    DhProfScope prof("dh_beam_history_logits", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_history_logits_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, group_max, gm_ld,
                       n_groups, group_cols, tokens, tok_ld, tok_row_mult, pos, rows_per_img, first_pos, ngram, penalty);
    DH_LAUNCH_CHECK();
}

// ---- history-dependent bans (min_len, bad_words_ids) in front of the row draw ---------------------------------------------------
// One workgroup per logits row, on the row geometry of beam_history_logits_kernel (history h[0 .. pos) = columns < pos of token row
// r * tok_row_mult; forced / idle rows of a prompted launch leave before the first barrier).  The banned phrases are one list for
// the whole launch: phrase w is words[word_off[w] .. word_off[w + 1]), 1 .. DH_BEAM_MAX_BAD_LEN ids.  Phases:
//   1. the last min(pos, DH_BEAM_MAX_BAD_LEN - 1) tokens of the history go to LDS (no phrase looks further back); flags cleared;
//   2. pos < min_len and 0 <= eos < V: one thread stores -inf to the <eos> column;
//   3. thread tid walks phrases tid, tid + 256, ...: a phrase of l ids with l - 1 <= pos whose first l - 1 ids equal the history's
//      last l - 1 tokens (compared from the phrase's last prefix id backwards: most phrases leave after one compare; l == 1 has
//      no prefix and always matches) stores -inf to the column of its last id.  A last id outside [0, V) is never a column;
//      prefix ids are compared as they are;
//   4. group_max != NULL: the repair of beam_history_logits_kernel's phase 3, same CONVENTION (exact fp32 maximum over the
//      group's REAL columns < V, pads never read, -inf for an all-banned group, groups without a store not written).
// Every store is -inf, which the penalty of beam_history_logits_kernel maps to itself: the two launches commute on the logits, and
// each leaves exact maxima behind, so they compose in either order.
__global__ __launch_bounds__(256) void beam_constrain_logits_kernel(
    float* logits, int ldl, int V, float* gmax, int gm_ld, int n_groups, int gcols, const int32_t* __restrict__ tokens, int tok_ld,
    int tok_row_mult, int pos, int rows_per_img, const int32_t* __restrict__ first_pos, int eos, int min_len,
    const int32_t* __restrict__ words, const int32_t* __restrict__ word_off, int n_words) {
    constexpr int NT = 256, MAXG = 1024, TAIL = DH_BEAM_MAX_BAD_LEN - 1;
    __shared__ int tail[TAIL];                       // tail[T - 1] is the row's latest token
    __shared__ int gflag[MAXG], glist[MAXG];
    __shared__ int s_ng;
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (first_pos && prompt_row_idle(first_pos, rc, rows_per_img, pos)) return;
    float* row = logits + (size_t)rc * ldl;
    const int32_t* h = tokens + (size_t)rc * tok_row_mult * tok_ld;
    const int T = pos < TAIL ? pos : TAIL;
    if (tid < T) tail[tid] = h[pos - T + tid];
    if (gmax)
        for (int g = tid; g < n_groups; g += NT) gflag[g] = 0;
    if (tid == 0) s_ng = 0;
    __syncthreads();
    auto ban = [&](int t) {               // column t (0 <= t < V <= n_groups * gcols) becomes -inf; its group is listed once
        row[t] = -INFINITY;
        if (gmax) {
            const int g = t / gcols;
            if (atomicExch(&gflag[g], 1) == 0) glist[atomicAdd(&s_ng, 1)] = g;
        }
    };
    if (tid == 0 && pos < min_len && eos >= 0 && eos < V) ban(eos);
    for (int w = tid; w < n_words; w += NT) {
        const int o = word_off[w], l = word_off[w + 1] - o;
        if (l < 1 || l > DH_BEAM_MAX_BAD_LEN || l - 1 > pos) continue;
        const int t = words[o + l - 1];
        if (t < 0 || t >= V) continue;
        bool eq = true;
        for (int k = 1; k < l && eq; ++k) eq = words[o + l - 1 - k] == tail[T - k];
        if (eq) ban(t);
    }
    if (gmax) {
        __threadfence_block();
        __syncthreads();
        // a list of single-token bans edits many groups of every row (50 singles: ~50 groups): each wave takes U listed groups at a
        // time and issues their U loads before the first reduction, so a trip costs one memory latency, not U
        constexpr int U = 4;
        const int ng = s_ng;
        for (int q0 = wave * U; q0 < ng; q0 += (NT / 64) * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool on = q0 + u < ng;                         // (wave-uniform)
                const int c = (on ? glist[q0 + u] : 0) * gcols + lane;
                v[u] = (on && lane < gcols && c < V) ? row[c] : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) v[u] = fmaxf(v[u], __shfl_xor(v[u], s, 64));
                if (lane == 0 && q0 + u < ng) gmax[(size_t)rc * gm_ld + glist[q0 + u]] = v[u];
            }
        }
    }
}

extern "C" int dh_beam_constrain_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                                        const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                                        const int32_t* first_pos, int eos_index, int min_len, const int32_t* words,
                                        const int32_t* word_off, int n_words, void* stream) {
    DH_REQUIRE(logits && tokens && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V && tok_row_mult >= 1);
    DH_REQUIRE(pos >= 0 && pos <= tok_ld && min_len >= 0);
    DH_REQUIRE(n_words >= 0 && n_words <= DH_BEAM_MAX_BAD_WORDS && (n_words == 0 || (words && word_off)));
    DH_REQUIRE(n_words > 0 || pos < min_len);                                  // nothing to ban: the caller makes no launch
    DH_REQUIRE(!group_max || (n_groups > 0 && n_groups <= 1024 && gm_ld >= n_groups && group_cols > 0 && group_cols <= 64 &&
                              (long long)n_groups * group_cols >= V));         // dh_beam_row_sample_groups' contract
    DH_REQUIRE(!first_pos || rows % rows_per_img == 0);
    DhProfScope prof("dh_beam_constrain_logits", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_constrain_logits_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, group_max, gm_ld,
                       n_groups, group_cols, tokens, tok_ld, tok_row_mult, pos, rows_per_img, first_pos, eos_index, min_len, words,
                       word_off, n_words);
    DH_LAUNCH_CHECK();
}

// ---- history-dependent biases (sequence_bias) in front of the row draw ----------------------------------------------------------
// One workgroup per logits row, on the row geometry of beam_constrain_logits_kernel (history h[0 .. pos) = columns < pos of token row
// r * tok_row_mult; forced / idle rows of a prompted launch leave before the first barrier).  The phrases are one list for the whole
// launch, STABLY SORTED BY LAST ID on the host: phrase w is words[word_off[w] .. word_off[w + 1]) with bias[w] (fp32), and run q is
// the phrases run_off[q] .. run_off[q + 1) -- all the phrases of one last id, in the order the caller listed them.  A column
// belongs to one run and a run to one thread, so no two threads read-modify-write one column.  Phases:
//   1. the last min(pos, DH_BEAM_MAX_BAD_LEN - 1) tokens of the history go to LDS; flags cleared;
//   2. thread tid walks runs tid, tid + 256, ...: it loads the run's column once, walks the run's phrases in order -- a phrase of
//      l ids with l - 1 <= pos whose first l - 1 ids equal the history's last l - 1 tokens fires (compared from the phrase's last
//      prefix id backwards; l == 1 always fires) -- and adds the bias of each one that fires, every addition its own
//      round-to-nearest fp32 add (__fadd_rn: never contracted, never re-associated), x = ((x + b1) + b2) ...; -inf stays -inf.  It
//      stores the column once if any phrase fired.  A last id outside [0, V) is never a column; a phrase whose last id is not its
//      run's (a list that was not sorted) is skipped, so the ownership holds whatever the list is;
//   3. group_max != NULL: the repair of beam_constrain_logits_kernel's phase 4, same CONVENTION (exact fp32 maximum over the
//      group's REAL columns < V, pads never read, groups without a store not written).  A raised column and a lowered one are the
//      same case: the group is read back.
__global__ __launch_bounds__(256) void beam_bias_logits_kernel(
    float* logits, int ldl, int V, float* gmax, int gm_ld, int n_groups, int gcols, const int32_t* __restrict__ tokens, int tok_ld,
    int tok_row_mult, int pos, int rows_per_img, const int32_t* __restrict__ first_pos, const int32_t* __restrict__ words,
    const int32_t* __restrict__ word_off, const float* __restrict__ bias, const int32_t* __restrict__ run_off, int n_words, int n_runs) {
    constexpr int NT = 256, MAXG = 1024, TAIL = DH_BEAM_MAX_BAD_LEN - 1;
    __shared__ int tail[TAIL];                       // tail[T - 1] is the row's latest token
    __shared__ int gflag[MAXG], glist[MAXG];
    __shared__ int s_ng;
    const int rc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (first_pos && prompt_row_idle(first_pos, rc, rows_per_img, pos)) return;
    float* row = logits + (size_t)rc * ldl;
    const int32_t* h = tokens + (size_t)rc * tok_row_mult * tok_ld;
    const int T = pos < TAIL ? pos : TAIL;
    if (tid < T) tail[tid] = h[pos - T + tid];
    if (gmax)
        for (int g = tid; g < n_groups; g += NT) gflag[g] = 0;
    if (tid == 0) s_ng = 0;
    __syncthreads();
    for (int q = tid; q < n_runs; q += NT) {
        const int w0 = run_off[q], w1 = run_off[q + 1];
        if (w0 < 0 || w1 > n_words || w0 >= w1) continue;
        const int o0 = word_off[w0], l0 = word_off[w0 + 1] - o0;
        if (l0 < 1 || l0 > DH_BEAM_MAX_BAD_LEN) continue;
        const int t = words[o0 + l0 - 1];                // the run's column
        if (t < 0 || t >= V) continue;
        float x = row[t];
        bool any = false;
        for (int w = w0; w < w1; ++w) {
            const int o = word_off[w], l = word_off[w + 1] - o;
            if (l < 1 || l > DH_BEAM_MAX_BAD_LEN || l - 1 > pos || words[o + l - 1] != t) continue;
            bool eq = true;
            for (int k = 1; k < l && eq; ++k) eq = words[o + l - 1 - k] == tail[T - k];
            if (eq) { x = __fadd_rn(x, bias[w]); any = true; }
        }
        if (any) {
            row[t] = x;
            if (gmax) {                   // (t < V <= n_groups * gcols) the column's group is listed once
                const int g = t / gcols;
                if (atomicExch(&gflag[g], 1) == 0) glist[atomicAdd(&s_ng, 1)] = g;
            }
        }
    }
    if (gmax) {
        __threadfence_block();
        __syncthreads();
        // a list of single-id biases edits many groups of every row: each wave takes U listed groups at a time and issues their U
        // loads before the first reduction, so a trip costs one memory latency, not U (beam_constrain_logits_kernel)
        constexpr int U = 4;
        const int ng = s_ng;
        for (int q0 = wave * U; q0 < ng; q0 += (NT / 64) * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool on = q0 + u < ng;                         // (wave-uniform)
                const int c = (on ? glist[q0 + u] : 0) * gcols + lane;
                v[u] = (on && lane < gcols && c < V) ? row[c] : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) v[u] = fmaxf(v[u], __shfl_xor(v[u], s, 64));
                if (lane == 0 && q0 + u < ng) gmax[(size_t)rc * gm_ld + glist[q0 + u]] = v[u];
            }
        }
    }
}

extern "C" int dh_beam_bias_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                                   const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                                   const int32_t* first_pos, const int32_t* words, const int32_t* word_off, const float* bias,
                                   const int32_t* run_off, int n_words, int n_runs, void* stream) {
    DH_REQUIRE(logits && tokens && rows > 0 && rows_per_img > 0 && V > 0 && ldl >= V && tok_row_mult >= 1);
    DH_REQUIRE(pos >= 0 && pos <= tok_ld);
    DH_REQUIRE(n_words >= 1 && n_words <= DH_BEAM_MAX_BAD_WORDS && words && word_off && bias && run_off);   // an empty list: no launch
    DH_REQUIRE(n_runs >= 1 && n_runs <= n_words);
    DH_REQUIRE(!group_max || (n_groups > 0 && n_groups <= 1024 && gm_ld >= n_groups && group_cols > 0 && group_cols <= 64 &&
                              (long long)n_groups * group_cols >= V));         // dh_beam_row_sample_groups' contract
    DH_REQUIRE(!first_pos || rows % rows_per_img == 0);
    DhProfScope prof("dh_beam_bias_logits", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_bias_logits_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, group_max, gm_ld,
                       n_groups, group_cols, tokens, tok_ld, tok_row_mult, pos, rows_per_img, first_pos, words, word_off, bias, run_off,
                       n_words, n_runs);
    DH_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------

template <int MB, bool PR, bool DT = false, bool LN = false>
__global__ __launch_bounds__(64) void beam_select_kernel(SelectParams p) {
    extern __shared__ int32_t stage[];
    __shared__ int ctok[MB * MB], cpar[MB * MB], keep[MB];
    __shared__ float cval[MB * MB], q[MB * MB];
    __shared__ uint8_t cend[MB * MB];
    __shared__ int s_n;
    __shared__ int32_t pki[MB * MB];
    __shared__ float pkv[MB * MB];
    const SelLds L{stage, ctok, cpar, keep, cval, q, cend, &s_n, pki, pkv};
    beam_select_image<MB, PR, DT, LN>(p, blockIdx.x, threadIdx.x, L);
}

template <bool PR, bool DT = false, bool LN = false>
static int select_launch(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                         float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                         int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                         int first, const int32_t* first_pos, int first_sets_ended, int write_pos, int t, int step_index,
                         float temperature, int eos_index, const float* noise, uint64_t seed,
                         const uint64_t* seed_ptr, int img0, void* stream, float* keys = nullptr, const float* len_w = nullptr,
                         int first_col = 0) {
    DH_REQUIRE(pick_idx && pick_val && tokens && vals && ended && parent && hparent && done && end_step);
    DH_REQUIRE(n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && tok_ld > 0 && t >= 0 && temperature > 0.f);
    DH_REQUIRE(!src || src_ld > t);
    DH_REQUIRE(!PR || first_pos);
    DH_REQUIRE(!LN || (len_w && keys && first_col >= 0));
    DhProfScope prof(LN ? "dh_beam_select_best_norm" : DT ? "dh_beam_select_best" : "dh_beam_select", 0.0, 0.0, stream);
    SelectParams p{pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step,
                   beam, first, first_sets_ended, write_pos, t, step_index, eos_index, img0, temperature, noise, seed, seed_ptr, first_pos,
                   keys, len_w, first_col};
    const size_t lds = (size_t)beam * (tok_ld + (src ? t : 0)) * sizeof(int32_t);
    DH_REQUIRE(lds <= 56 * 1024);                         // beam * (tok_ld + t) ints of staging next to the candidate arrays
    if (beam <= 16) hipLaunchKernelGGL((beam_select_kernel<16, PR, DT, LN>), dim3(n_img), dim3(64), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((beam_select_kernel<DH_BEAM_MAX_BEAMS, PR, DT, LN>), dim3(n_img), dim3(64), lds, (hipStream_t)stream, p);   // beam.py:7-9: any beam_size <= top_k
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_select(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                              float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                              int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                              int first, int first_sets_ended, int write_pos, int t, int step_index,
                              float temperature, int eos_index, const float* noise, uint64_t seed,
                              const uint64_t* seed_ptr, int img0, void* stream) {
    return select_launch<false>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step, n_img, beam,
                                first, nullptr, first_sets_ended, write_pos, t, step_index, temperature, eos_index, noise, seed, seed_ptr, img0,
                                stream);
}

extern "C" int dh_beam_select_prompted(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                                       float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                                       int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                                       const int32_t* first_pos, int first_sets_ended, int write_pos, int t, int step_index,
                                       float temperature, int eos_index, const float* noise, uint64_t seed,
                                       const uint64_t* seed_ptr, int img0, void* stream) {
    return select_launch<true>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step, n_img, beam,
                               0, first_pos, first_sets_ended, write_pos, t, step_index, temperature, eos_index, noise, seed, seed_ptr, img0,
                               stream);
}

// The deterministic select of search="beam" (the DT instantiations): dense with first_pos == NULL and the launch-wide `first`, prompted
// with first_pos (`first` is not read then).  No noise, no seed, no temperature: the rank is on the fp32 scores themselves.
extern "C" int dh_beam_select_best(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                                   float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                                   int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                                   int first, const int32_t* first_pos, int first_sets_ended, int write_pos, int t, int step_index,
                                   int eos_index, void* stream) {
    if (first_pos)
        return select_launch<true, true>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step, n_img,
                                         beam, 0, first_pos, first_sets_ended, write_pos, t, step_index, 1.f, eos_index, nullptr, 0ull, nullptr,
                                         0, stream);
    return select_launch<false, true>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step, n_img,
                                      beam, first, nullptr, first_sets_ended, write_pos, t, step_index, 1.f, eos_index, nullptr, 0ull, nullptr,
                                      0, stream);
}

// dh_beam_select_best with length normalisation (the LN instantiations): the `beam` candidates with the largest key = score *
// len_w[L] stay -- len_w fp32 [tok_ld + 1], len_w[0] = 1, L = write_pos + 1 - first_col (prompted: - first_pos[img]) for a live
// candidate; an ended beam's candidate carries the key it was kept with.  keys fp32 [rows] receives the kept candidates' keys (a first
// step: pick_val * len_w[L]); vals keeps the raw cumulative scores.  Everything else is dh_beam_select_best's.
extern "C" int dh_beam_select_best_norm(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                                        float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                                        int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                                        int first, const int32_t* first_pos, int first_col, const float* len_w, int first_sets_ended,
                                        int write_pos, int t, int step_index, int eos_index, void* stream) {
    if (first_pos)
        return select_launch<true, true, true>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step,
                                               n_img, beam, 0, first_pos, first_sets_ended, write_pos, t, step_index, 1.f, eos_index, nullptr,
                                               0ull, nullptr, 0, stream, keys, len_w, first_col);
    return select_launch<false, true, true>(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step,
                                            n_img, beam, first, nullptr, first_sets_ended, write_pos, t, step_index, 1.f, eos_index, nullptr,
                                            0ull, nullptr, 0, stream, keys, len_w, first_col);
}

// ---- early_stopping: the finished-hypothesis pool of search="beam" -------------------------------------------------------------------
template <int MB, bool PR>
__global__ __launch_bounds__(64) void beam_select_pool_kernel(SelectParams p) {
    extern __shared__ int32_t stage[];
    __shared__ int ctok[MB * MB], cpar[MB * MB], keep[MB], ord[2 * MB], offer[MB];
    __shared__ float cval[MB * MB], q[MB * MB];
    __shared__ uint8_t cend[MB * MB];
    __shared__ int s_n;
    __shared__ int32_t pki[MB * MB];
    __shared__ float pkv[MB * MB];
    const SelLds L{stage, ctok, cpar, keep, cval, q, cend, &s_n, pki, pkv, ord, offer};
    beam_select_image<MB, PR, true, true, true>(p, blockIdx.x, threadIdx.x, L);
}

// dh_beam_select_best_norm with a finished-hypothesis pool (the PL instantiations; beam_pool_tail has the rules): a candidate whose
// token is <eos> never takes a beam slot -- among the first `beam` ranks it is offered to the image's pool --, the `beam` best others
// stay as live beams, and a slot nothing is left for is dead (ended = 1, -inf).  `ended` therefore marks dead slots only.  The pool
// rows have the token table's stride.  stop_when_full: 1 = early_stopping=True, 0 = False.
extern "C" int dh_beam_select_pool(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                                   float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                                   int32_t* hparent, uint8_t* done, int32_t* end_step, int32_t* pool_tokens, float* pool_keys,
                                   float* pool_vals, int32_t* pool_len, int32_t* pool_n, int n_img, int beam,
                                   int first, const int32_t* first_pos, int first_col, const float* len_w, int stop_when_full,
                                   int write_pos, int t, int step_index, int eos_index, void* stream) {
    DH_REQUIRE(pick_idx && pick_val && tokens && vals && keys && ended && parent && hparent && done && end_step && len_w);
    DH_REQUIRE(pool_tokens && pool_keys && pool_vals && pool_len && pool_n);
    DH_REQUIRE(n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && tok_ld > 0 && t >= 0 && first_col >= 0 && step_index >= 0);
    DH_REQUIRE(write_pos >= 0 && write_pos < tok_ld);    // an offered hypothesis holds <eos> at write_pos
    DH_REQUIRE(stop_when_full == 0 || stop_when_full == 1);
    DH_REQUIRE(!src || src_ld > t);
    DhProfScope prof("dh_beam_select_pool", 0.0, 0.0, stream);
    SelectParams p{pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step,
                   beam, first_pos ? 0 : first, 0, write_pos, t, step_index, eos_index, 0, 1.f, nullptr, 0ull, nullptr, first_pos,
                   keys, len_w, first_col, pool_tokens, pool_keys, pool_vals, pool_len, pool_n, stop_when_full};
    const size_t lds = (size_t)beam * (tok_ld + (src ? t : 0)) * sizeof(int32_t);
    DH_REQUIRE(lds <= 56 * 1024);
    const dim3 grid(n_img), block(64);
    if (first_pos) {
        if (beam <= 16) hipLaunchKernelGGL((beam_select_pool_kernel<16, true>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((beam_select_pool_kernel<DH_BEAM_MAX_BEAMS, true>), grid, block, lds, (hipStream_t)stream, p);
    } else {
        if (beam <= 16) hipLaunchKernelGGL((beam_select_pool_kernel<16, false>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((beam_select_pool_kernel<DH_BEAM_MAX_BEAMS, false>), grid, block, lds, (hipStream_t)stream, p);
    }
    DH_LAUNCH_CHECK();
}

// ---- num_beam_groups: diverse groups of beams under search="beam" ---------------------------------------------------------------------
template <int MB, bool PR>
__global__ __launch_bounds__(64) void beam_select_groups_kernel(SelectParams p) {
    extern __shared__ int32_t stage[];
    __shared__ int ctok[MB * MB], cpar[MB * MB], keep[MB];
    __shared__ float cval[MB * MB], q[MB * MB];
    __shared__ uint8_t cend[MB * MB];
    __shared__ int s_n;
    __shared__ int32_t pki[MB * MB];
    __shared__ float pkv[MB * MB];
    static_assert(MB * MB >= 2 * MB + 1, "`said` and the group starts fit the pick indices' array");
    // the picks are consumed when the candidate list stands: their two arrays then hold the penalised keys and the tokens taken
    const SelLds L{stage, ctok, cpar, keep, cval, q, cend, &s_n, pki, pkv, nullptr, nullptr, pkv, pki};
    beam_select_image<MB, PR, true, true, false, true>(p, blockIdx.x, threadIdx.x, L);
}

// dh_beam_select_best_norm over n_groups groups of beam / n_groups slots each (the GR instantiations; beam_group_tail has the rules):
// group g ranks the candidates of its own slots' rows -- a first step: of the image's one row -- by key - diversity_penalty * (times the
// token was taken at this position by the groups before it), keeps the best beam / n_groups of them in its slots, and what is stored
// (vals, keys) is not penalised.  len_w is the table of ones without a length penalty.  Everything else is dh_beam_select_best_norm's.
extern "C" int dh_beam_select_groups(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                                     float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                                     int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                                     int first, const int32_t* first_pos, int first_col, const float* len_w, int first_sets_ended,
                                     int write_pos, int t, int step_index, int eos_index, int n_groups, float diversity_penalty,
                                     void* stream) {
    DH_REQUIRE(pick_idx && pick_val && tokens && vals && ended && parent && hparent && done && end_step);
    DH_REQUIRE(n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && tok_ld > 0 && t >= 0);
    DH_REQUIRE(!src || src_ld > t);
    DH_REQUIRE(len_w && keys && first_col >= 0);
    DH_REQUIRE(n_groups >= 1 && beam % n_groups == 0);
    DH_REQUIRE(diversity_penalty > 0.f && diversity_penalty < INFINITY);
    DhProfScope prof("dh_beam_select_groups", 0.0, 0.0, stream);
    SelectParams p{pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step,
                   beam, first_pos ? 0 : first, first_sets_ended, write_pos, t, step_index, eos_index, 0, 1.f, nullptr, 0ull, nullptr, first_pos,
                   keys, len_w, first_col};
    p.n_groups = n_groups;
    p.diversity = diversity_penalty;
    const size_t lds = (size_t)beam * (tok_ld + (src ? t : 0)) * sizeof(int32_t);
    DH_REQUIRE(lds <= 56 * 1024);
    const dim3 grid(n_img), block(64);
    if (first_pos) {
        if (beam <= 16) hipLaunchKernelGGL((beam_select_groups_kernel<16, true>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((beam_select_groups_kernel<DH_BEAM_MAX_BEAMS, true>), grid, block, lds, (hipStream_t)stream, p);
    } else {
        if (beam <= 16) hipLaunchKernelGGL((beam_select_groups_kernel<16, false>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((beam_select_groups_kernel<DH_BEAM_MAX_BEAMS, false>), grid, block, lds, (hipStream_t)stream, p);
    }
    DH_LAUNCH_CHECK();
}

// One wave per image, lane j = pool entry j and live slot j.  The result is the pool with -- for an image that is not done -- its live
// slots (ended == 0) offered in slot order through the select's insertion rule: that is the stable descending order of "the pool's
// entries, then the live slots" by key, cut at `beam` (what falls off during the insertions is never among the best `beam`).  So an
// entry's output slot is a count: the entries with a larger key, plus those with an equal key that stand in front of it.  Fewer than
// `beam` entries: the slots that were not offered follow in slot order at score -inf.  Nothing is written to the pool or the state.
__global__ __launch_bounds__(64) void beam_finalize_pool_kernel(
    const int32_t* __restrict__ tokens, int tok_ld, const float* __restrict__ keys, const uint8_t* __restrict__ ended,
    const uint8_t* __restrict__ done, const int32_t* __restrict__ pool_tokens, const float* __restrict__ pool_keys,
    const int32_t* __restrict__ pool_len, const int32_t* __restrict__ pool_n, int32_t* __restrict__ out_tokens, int out_ld,
    int32_t* __restrict__ out_len, float* __restrict__ out_score, int32_t* __restrict__ out_index, int32_t* __restrict__ out_drawn,
    int32_t* __restrict__ out_row_len, int beam, int full_len, int pad_index) {
    __shared__ int s_from[DH_BEAM_MAX_BEAMS], s_len[DH_BEAM_MAX_BEAMS];      // per output slot: source (pool entry j: -1 - j; slot j: j), length
    const int img = blockIdx.x, lane = threadIdx.x, B = beam, base = img * B;
    const int cap = min(out_ld, tok_ld);
    const int n_pool = min(max(pool_n[img], 0), B);
    const bool in_pool = lane < n_pool;
    const bool live = lane < B && !done[img] && !ended[base + lane];
    float pk = in_pool ? pool_keys[base + lane] : -INFINITY;
    float lk = live ? keys[base + lane] : -INFINITY;
    if (!(pk == pk)) pk = -INFINITY;                      // (a NaN orders like -inf: the slots stay a permutation)
    if (!(lk == lk)) lk = -INFINITY;
    const int plen = in_pool ? min(max(pool_len[base + lane], 0), cap) : 0;
    const int llen = min(max(full_len, 0), cap);
    int prank = lane, lrank = 0;                          // the pool is sorted: entry j has j entries in front of it
    for (int j = 0; j < B; ++j) {
        const float opk = __shfl(pk, j), olk = __shfl(lk, j);
        const bool o_pool = j < n_pool, o_live = __shfl((int)live, j) != 0;
        prank += o_live && olk > pk;
        lrank += (o_pool && opk >= lk) + (o_live && (olk > lk || (olk == lk && j < lane)));
    }
    const int n_live = __popcll(__ballot(live));
    const int total = n_pool + n_live;
    // the slots that were not offered, in slot order, behind the entries
    const unsigned long long idle = __ballot(lane < B && !live);
    const int frank = total + __popcll(idle & ((1ull << lane) - 1ull));
    if (lane < B) { s_from[lane] = lane; s_len[lane] = 0; }     // (a pool that is not sorted leaves a slot out: never an index from nowhere)
    __syncthreads();
    if (in_pool && prank < B) {
        s_from[prank] = -1 - lane; s_len[prank] = plen;
        out_score[base + prank] = pk; out_index[base + prank] = -1; out_len[base + prank] = plen;
    }
    if (live && lrank < B) {
        s_from[lrank] = lane; s_len[lrank] = llen;
        out_score[base + lrank] = lk; out_index[base + lrank] = lane; out_len[base + lrank] = llen;
    }
    if (lane < B && !live && frank < B) {
        s_from[frank] = lane; s_len[frank] = llen;
        out_score[base + frank] = -INFINITY; out_index[base + frank] = lane; out_len[base + frank] = llen;
    }
    __syncthreads();
    if (lane == 0) { out_drawn[img] = 0; out_row_len[img] = s_len[0]; }
    for (int s = 0; s < B; ++s) {
        const int from = s_from[s], len = s_len[s];
        const int32_t* __restrict__ row = from < 0 ? pool_tokens + (size_t)(base + (-1 - from)) * tok_ld : tokens + (size_t)(base + from) * tok_ld;
        int32_t* __restrict__ dst = out_tokens + (size_t)(base + s) * out_ld;
        for (int i = lane; i < out_ld; i += 64) dst[i] = i < len ? row[i] : pad_index;
    }
}

extern "C" int dh_beam_finalize_pool(const int32_t* tokens, int tok_ld, const float* keys, const uint8_t* ended, const uint8_t* done,
                                     const int32_t* pool_tokens, const float* pool_keys, const int32_t* pool_len, const int32_t* pool_n,
                                     int32_t* out_tokens, int out_ld, int32_t* out_len, float* out_score, int32_t* out_index,
                                     int32_t* out_drawn, int32_t* out_row_len, int n_img, int beam, int full_len, int pad_index,
                                     void* stream) {
    DH_REQUIRE(tokens && keys && ended && done && pool_tokens && pool_keys && pool_len && pool_n);
    DH_REQUIRE(out_tokens && out_len && out_score && out_index && out_drawn && out_row_len);
    DH_REQUIRE(n_img > 0 && tok_ld > 0 && out_ld > 0 && full_len >= 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS);
    DhProfScope prof("dh_beam_finalize_pool", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_finalize_pool_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, tokens, tok_ld, keys, ended, done,
                       pool_tokens, pool_keys, pool_len, pool_n, out_tokens, out_ld, out_len, out_score, out_index, out_drawn, out_row_len,
                       beam, full_len, pad_index);
    DH_LAUNCH_CHECK();
}

// ---- the reference's METHOD surface (deephumor/models/beam.py:32-108), one kernel per method ------------------------------------
// BeamSearchHelper.filter_top_k / sample_k_indices / filter_by_indices / process_logits as the reference's own generate() loops
// call them (rnn_models.py:87-128, transformers.py:532-569): host-driven, one image at a time, tensors of the reference's shapes
// and dtypes (int64 indices, fp32 values, in-place -inf filter).  The batched decode engine above does not use them.

__device__ __forceinline__ float key2f(uint32_t k) {           // inverse of f2key
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// beam.py:34-36: logits[logits < kth_largest] = -inf (strict: ties at the threshold stay), logits[:, unk] = -inf
__global__ __launch_bounds__(256) void beam_filter_topk_kernel(float* __restrict__ logits, int ldl, int V, int top_k, int unk) {
    __shared__ int hist[4 * 256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k, wtot[4];
    const int tid = threadIdx.x, hw = tid >> 6;
    float* row = logits + (size_t)blockIdx.x * ldl;
    if (tid == 0) { s_prefix = 0u; s_k = top_k; }
    uint32_t mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 1024; i += 256) hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (int i = tid; i < V; i += 256) {
            const uint32_t key = f2key(row[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[hw * 256 + ((key >> shift) & 255u)], 1);
        }
        __syncthreads();
        radix_pick_digit(hist, 4, shift, prefix, &s_prefix, &s_k, wtot);
        mask |= 0xFFu << shift;
    }
    const float thr = key2f(s_prefix);                          // the k-th largest value of the row
    for (int i = tid; i < V; i += 256)
        if (row[i] < thr || i == unk) row[i] = -INFINITY;
}

// beam.py:39-48: p = softmax(x / T); torch.multinomial(p, k) without replacement == the k largest of p / Exp(1) noise, in
// descending order (CPU torch).  k rounds of a block arg-max (ties -> lower index) over the whole row.
__global__ __launch_bounds__(256) void beam_sample_k_kernel(const float* __restrict__ x, int ld, int V, int k, float temperature,
                                                            const float* __restrict__ noise, int noise_ld, uint64_t seed,
                                                            const uint64_t* __restrict__ seed_ptr, int stream_id, int draw,
                                                            int64_t* __restrict__ out, int32_t* __restrict__ err) {
    __shared__ float red[256];
    __shared__ float rq[256];
    __shared__ int ri[256];
    __shared__ int picked[64];
    const int tid = threadIdx.x, r = blockIdx.x;
    const float* row = x + (size_t)r * ld;
    float m = -INFINITY;
    for (int i = tid; i < V; i += 256) m = fmaxf(m, row[i] / temperature);
    m = block_reduce_256(m, red, true);
    if (m == -INFINITY) {                                       // softmax of an all -inf row is NaN: torch raises
        if (tid == 0) atomicOr(err, DH_BEAM_ERR_ALL_FILTERED);
        for (int j = tid; j < k; j += 256) out[(size_t)r * k + j] = 0;
        return;
    }
    float s = 0.f, cnt = 0.f;
    for (int i = tid; i < V; i += 256) { const float e = expf(row[i] / temperature - m); s += e; cnt += e > 0.f ? 1.f : 0.f; }
    s = block_reduce_256(s, red, false);
    cnt = block_reduce_256(cnt, red, false);
    if (tid == 0 && cnt < (float)k) atomicOr(err, DH_BEAM_ERR_TOO_FEW);      // "not enough non-negative category to sample"
    const uint64_t sd = seed ^ (seed_ptr ? *seed_ptr : 0ull);
    for (int round = 0; round < k; ++round) {
        float bq = -1.f; int bi = 0x7FFFFFFF;
        for (int i = tid; i < V; i += 256) {
            bool taken = false;
            for (int j = 0; j < round; ++j) taken |= picked[j] == i;
            if (taken) continue;
            const float nz = noise ? noise[(size_t)r * noise_ld + i] : philox_exp1(sd, (uint32_t)stream_id, (uint32_t)draw, 3u, (uint32_t)r, (uint32_t)i);
            const float q = (expf(row[i] / temperature - m) / s) / nz;
            if (q > bq) { bq = q; bi = i; }                     // ascending i: the first (lowest) index wins a tie
        }
        rq[tid] = bq; ri[tid] = bi;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) {
                const float oq = rq[tid + st]; const int oi = ri[tid + st];
                if (oq > rq[tid] || (oq == rq[tid] && oi < ri[tid])) { rq[tid] = oq; ri[tid] = oi; }
            }
            __syncthreads();
        }
        if (tid == 0) { picked[round] = ri[0]; out[(size_t)r * k + round] = ri[0] == 0x7FFFFFFF ? 0 : ri[0]; }
        __syncthreads();
    }
}

// beam.py:50-53: torch.gather(values, 1, indices)
__global__ void beam_gather_kernel(const float* __restrict__ values, int ld, int V, const int64_t* __restrict__ indices, int k,
                                   float* __restrict__ out, int total, int32_t* __restrict__ err) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t i = indices[t];
    if (i < 0 || i >= V) { if (err) atomicOr(err, DH_BEAM_ERR_OVERFLOW); out[t] = 0.f; return; }
    out[t] = values[(size_t)(t / k) * ld + i];
}

// beam.py:78-106: log_softmax over each row's gathered picks, then the candidate expansion -- a live beam contributes `beam`
// candidates, an ended one a single candidate with token 0 / score 0 -- with the new has_ended flags and the repeated sequences.
__global__ __launch_bounds__(64) void beam_expand_kernel(const int64_t* __restrict__ ind, const float* __restrict__ gathered,
                                                         const uint8_t* __restrict__ ended, const int64_t* __restrict__ seqs, int seq_len,
                                                         const float* __restrict__ vals, int val_w, int n, int beam, int eos,
                                                         int64_t* __restrict__ prev_seqs, float* __restrict__ prev_vals,
                                                         int64_t* __restrict__ new_ind, float* __restrict__ new_val,
                                                         uint8_t* __restrict__ new_ended) {
    const int lane = threadIdx.x;
    int total = 0;
    for (int b = 0; b < n; ++b) total += ended[b] ? 1 : beam;
    for (int c = lane; c < total; c += 64) {
        int b = 0, off = 0;
        for (;;) { const int w = ended[b] ? 1 : beam; if (c < off + w) break; off += w; ++b; }
        const int j = c - off;
        const bool was = ended[b] != 0;
        float mx = -INFINITY;
        for (int u = 0; u < beam; ++u) mx = fmaxf(mx, gathered[(size_t)b * beam + u]);
        float se = 0.f;
        for (int u = 0; u < beam; ++u) se += expf(gathered[(size_t)b * beam + u] - mx);
        const int64_t tok = was ? 0 : ind[(size_t)b * beam + j];
        new_ind[c] = tok;
        new_val[c] = was ? 0.f : (gathered[(size_t)b * beam + j] - mx) - logf(se);
        new_ended[c] = (uint8_t)(was || tok == eos);
        for (int i = 0; i < seq_len; ++i) prev_seqs[(size_t)c * seq_len + i] = seqs[(size_t)b * seq_len + i];
        for (int i = 0; i < val_w; ++i) prev_vals[(size_t)c * val_w + i] = vals[(size_t)b * val_w + i];
    }
}

extern "C" int dh_beam_filter_top_k(float* logits, int ldl, int V, int rows, int top_k, int unk_index, void* stream) {
    DH_REQUIRE(logits && rows > 0 && V > 0 && ldl >= V && top_k >= 1 && top_k <= V);
    DhProfScope prof("dh_beam_filter_top_k", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_filter_topk_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, top_k, unk_index);
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_sample_k(const float* x, int ld, int V, int rows, int k, float temperature, const float* noise, int noise_ld,
                                uint64_t seed, const uint64_t* seed_ptr, int stream_id, int draw, int64_t* out, int32_t* err,
                                void* stream) {
    DH_REQUIRE(x && out && err && rows > 0 && V > 0 && ld >= V && k >= 1 && k <= 64 && k <= V && temperature > 0.f);
    DH_REQUIRE(!noise || noise_ld >= V);
    DhProfScope prof("dh_beam_sample_k", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_sample_k_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ld, V, k, temperature, noise, noise_ld,
                       seed, seed_ptr, stream_id, draw, out, err);
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_gather(const float* values, int ld, int V, const int64_t* indices, int k, float* out, int rows, int32_t* err,
                              void* stream) {
    DH_REQUIRE(values && indices && out && rows > 0 && k > 0 && V > 0 && ld >= V);
    DhProfScope prof("dh_beam_gather", 0.0, 0.0, stream);
    const int total = rows * k;
    hipLaunchKernelGGL(beam_gather_kernel, dim3(dh_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, values, ld, V, indices, k, out,
                       total, err);
    DH_LAUNCH_CHECK();
}

extern "C" int dh_beam_expand(const int64_t* new_ind, const float* gathered, const uint8_t* ended, const int64_t* seqs, int seq_len,
                              const float* vals, int val_width, int n_rows, int beam, int eos_index, int64_t* prev_seqs,
                              float* prev_vals, int64_t* out_ind, float* out_val, uint8_t* out_ended, void* stream) {
    DH_REQUIRE(new_ind && gathered && ended && seqs && vals && prev_seqs && prev_vals && out_ind && out_val && out_ended);
    DH_REQUIRE(n_rows > 0 && n_rows <= 1024 && beam >= 1 && beam <= 64 && seq_len >= 0 && val_width >= 1);
    DhProfScope prof("dh_beam_expand", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_expand_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, new_ind, gathered, ended, seqs, seq_len, vals,
                       val_width, n_rows, beam, eos_index, prev_seqs, prev_vals, out_ind, out_val, out_ended);
    DH_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void beam_finalize_kernel(
    const int32_t* __restrict__ tokens, int tok_ld, const float* __restrict__ vals, const uint8_t* __restrict__ done,
    const int32_t* __restrict__ end_step, int32_t* __restrict__ out, int out_ld, int32_t* __restrict__ out_len,
    int beam, int len_bias_done, int full_len, int pad_index, float temperature, const float* __restrict__ noise,
    uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0) {
    const int img = blockIdx.x, lane = threadIdx.x, base = img * beam;
    // ind = multinomial(softmax(vals / T), 1) == arg-max of p / Exp(1) (first index on ties)
    float x = lane < beam ? vals[base + lane] / temperature : -INFINITY;
    const float m = wave_max(x);
    float e = lane < beam ? expf(x - m) : 0.f;
    const float s = wave_sum(e);
    float qq = -1.f;
    if (lane < beam) {
        const float nz = noise ? noise[(size_t)img * beam + lane]
                               : philox_exp1(seed ^ (seed_ptr ? *seed_ptr : 0ull), (uint32_t)(img0 + img), 0xFFFFFFFFu, 2u, 0u, (uint32_t)lane);
        qq = (e / s) / nz;
    }
    const float best = wave_max(qq);
    const unsigned long long bal = __ballot(qq == best && lane < beam);
    const int ind = max(__ffsll((long long)bal) - 1, 0);          // (NaN scores: no lane equals the maximum -- never index row -1)
    int len = done[img] ? end_step[img] + len_bias_done : full_len;
    len = min(len, min(out_ld, tok_ld));
    for (int i = lane; i < out_ld; i += 64)
        out[(size_t)img * out_ld + i] = i < len ? tokens[(size_t)(base + ind) * tok_ld + i] : pad_index;
    if (lane == 0) out_len[img] = len;
}

extern "C" int dh_beam_finalize(const int32_t* tokens, int tok_ld, const float* vals, const uint8_t* done,
                                const int32_t* end_step, int32_t* out, int out_ld, int32_t* out_len,
                                int n_img, int beam, int len_bias_done, int full_len, int pad_index,
                                float temperature, const float* noise, uint64_t seed, const uint64_t* seed_ptr, int img0,
                                void* stream) {
    DH_REQUIRE(tokens && vals && done && end_step && out && out_len && n_img > 0);
    DH_REQUIRE(beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && temperature > 0.f);
    DhProfScope prof("dh_beam_finalize", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, tokens, tok_ld, vals,
                       done, end_step, out, out_ld, out_len, beam, len_bias_done, full_len, pad_index,
                       temperature, noise, seed, seed_ptr, img0);
    DH_LAUNCH_CHECK();
}

// ---- n-best finalisation: every beam of every image, ordered by score ---------------------------------------------------------
// One wave per image, lane = beam (beam <= DH_BEAM_MAX_BEAMS = one wave).  The final draw is beam_finalize_kernel's, statement for
// statement (same softmax, same Philox counters, same `noise` override), so out_drawn names the beam the plain call copies.  Every
// lane then ranks its own score among the image's beams with wave shuffles (registers only): slot = #beams with a larger score +
// #equal-score beams with a smaller engine index -- stable and descending; a NaN score orders like -inf, so the slots are always a
// permutation and the dead beams of DH_BEAM_ERR_TOO_FEW (score -inf) come last.  The rows are copied beam by beam the way the plain
// kernel copies the drawn one (columns < row_len from the token table, the rest pad_index), 64 columns per round; the same round
// looks for the row's first eos_index at or after the image's first generated column (ballot + find-first).
__global__ __launch_bounds__(64) void beam_finalize_beams_kernel(
    const int32_t* __restrict__ tokens, int tok_ld, const float* __restrict__ vals, const uint8_t* __restrict__ done,
    const int32_t* __restrict__ end_step, int32_t* __restrict__ out_tokens, int out_ld, int32_t* __restrict__ out_len,
    float* __restrict__ out_score, int32_t* __restrict__ out_index, int32_t* __restrict__ out_drawn, int32_t* __restrict__ out_row_len,
    int beam, int len_bias_done, int full_len, int pad_index, int eos_index, int pos, const int32_t* __restrict__ first_pos,
    float temperature, const float* __restrict__ noise, uint64_t seed, const uint64_t* __restrict__ seed_ptr, int img0) {
    const int img = blockIdx.x, lane = threadIdx.x, base = img * beam;
    const float score = lane < beam ? vals[base + lane] : -INFINITY;
    // ind = multinomial(softmax(vals / T), 1) == arg-max of p / Exp(1) (first index on ties): as beam_finalize_kernel
    float x = lane < beam ? score / temperature : -INFINITY;
    const float m = wave_max(x);
    float e = lane < beam ? expf(x - m) : 0.f;
    const float s = wave_sum(e);
    float qq = -1.f;
    if (lane < beam) {
        const float nz = noise ? noise[(size_t)img * beam + lane]
                               : philox_exp1(seed ^ (seed_ptr ? *seed_ptr : 0ull), (uint32_t)(img0 + img), 0xFFFFFFFFu, 2u, 0u, (uint32_t)lane);
        qq = (e / s) / nz;
    }
    const float best = wave_max(qq);
    const unsigned long long bal = __ballot(qq == best && lane < beam);
    const int ind = max(__ffsll((long long)bal) - 1, 0);
    int len = done[img] ? end_step[img] + len_bias_done : full_len;
    len = min(len, min(out_ld, tok_ld));
    // rank of my score among the image's beams (lanes >= beam take no part: they are never compared against, j < beam)
    const float key = score == score ? score : -INFINITY;
    int rank = 0;
    for (int j = 0; j < beam; ++j) {
        const float o = __shfl(key, j);
        rank += (o > key) || (o == key && j < lane);
    }
    if (lane < beam) {
        out_score[base + rank] = score;
        out_index[base + rank] = lane;
    }
    const int drawn = __shfl(rank, ind);
    if (lane == 0) { out_drawn[img] = drawn; out_row_len[img] = len; }
    const int p0 = first_pos ? first_pos[img] : pos;
    for (int b = 0; b < beam; ++b) {
        const int slot = __shfl(rank, b);
        const int32_t* __restrict__ src = tokens + (size_t)(base + b) * tok_ld;
        int32_t* __restrict__ dst = out_tokens + (size_t)(base + slot) * out_ld;
        int eos_at = -1;                                    // (wave-uniform)
        for (int c0 = 0; c0 < out_ld; c0 += 64) {
            const int i = c0 + lane;
            const int tok = i < len ? src[i] : pad_index;
            if (i < out_ld) dst[i] = tok;
            const unsigned long long hit = __ballot(i < len && i >= p0 && tok == eos_index);
            if (eos_at < 0 && hit) eos_at = c0 + __ffsll((long long)hit) - 1;
        }
        if (lane == 0) out_len[base + slot] = eos_at >= 0 ? eos_at + 1 : len;      // (eos_at < len: never past the row)
    }
}

extern "C" int dh_beam_finalize_beams(const int32_t* tokens, int tok_ld, const float* vals, const uint8_t* done,
                                      const int32_t* end_step, int32_t* out_tokens, int out_ld, int32_t* out_len,
                                      float* out_score, int32_t* out_index, int32_t* out_drawn, int32_t* out_row_len,
                                      int n_img, int beam, int len_bias_done, int full_len, int pad_index, int eos_index,
                                      int pos, const int32_t* first_pos, float temperature, const float* noise, uint64_t seed,
                                      const uint64_t* seed_ptr, int img0, void* stream) {
    DH_REQUIRE(tokens && vals && done && end_step && out_tokens && out_len && out_score && out_index && out_drawn && out_row_len);
    DH_REQUIRE(n_img > 0 && tok_ld > 0 && out_ld > 0 && pos >= 0);
    DH_REQUIRE(beam >= 1 && beam <= DH_BEAM_MAX_BEAMS && temperature > 0.f);
    DhProfScope prof("dh_beam_finalize_beams", 0.0, 0.0, stream);
    hipLaunchKernelGGL(beam_finalize_beams_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, tokens, tok_ld, vals,
                       done, end_step, out_tokens, out_ld, out_len, out_score, out_index, out_drawn, out_row_len, beam,
                       len_bias_done, full_len, pad_index, eos_index, pos, first_pos, temperature, noise, seed, seed_ptr, img0);
    DH_LAUNCH_CHECK();
}

// ---- return_attention: every kept beam's attention maps, through the ancestor table ----------------------------------------------
// out[i, j, c, :] = attn_w[c, src[i * beam + index[i, j], c], :] for c < len[i, j], else 0: slot j of image i holds engine beam
// index[i, j] (dh_beam_finalize_beams' out_index / out_len), and position c of that beam's history was computed by the logical row
// its src row names -- the indirection the KV cache is read through, so no map is ever copied when beams are shuffled.
// One workgroup of 64 lanes per (slot, column c); a src entry outside [0, rows_total) gives a zero row, never a foreign read.
__global__ __launch_bounds__(64) void beam_gather_attention_kernel(const float* __restrict__ attn_w, const int32_t* __restrict__ src, int src_ld,
                                                                    const int32_t* __restrict__ index, const int32_t* __restrict__ len,
                                                                    float* __restrict__ out, int beam, int T, int rows_total, int S) {
    const int slot = blockIdx.x, c = blockIdx.y, img = slot / beam, lane = threadIdx.x;
    float* dst = out + ((size_t)slot * T + c) * S;
    const int b = index[slot];
    int row = -1;
    if (c < len[slot] && b >= 0 && b < beam) row = src[(size_t)(img * beam + b) * src_ld + c];
    if (row < 0 || row >= rows_total) {
        for (int s = lane; s < S; s += 64) dst[s] = 0.f;
        return;
    }
    const float* from = attn_w + ((size_t)c * rows_total + row) * S;
    for (int s = lane; s < S; s += 64) dst[s] = from[s];
}

extern "C" int dh_beam_gather_attention(const float* attn_w, const int32_t* src, int src_ld, const int32_t* index, const int32_t* len,
                                        float* out, int n_img, int beam, int T, int n_pos, int rows_total, int S, void* stream) {
    DH_REQUIRE(attn_w && src && index && len && out && n_img > 0 && beam >= 1 && beam <= DH_BEAM_MAX_BEAMS);
    DH_REQUIRE(T > 0 && T <= n_pos && src_ld >= T && S > 0 && rows_total >= n_img * beam && T <= 65535);
    DhProfScope prof("dh_beam_gather_attention", 0.0, 8.0 * n_img * beam * T * S, stream);
    hipLaunchKernelGGL(beam_gather_attention_kernel, dim3(n_img * beam, T), dim3(64), 0, (hipStream_t)stream, attn_w, src, src_ld, index, len,
                       out, beam, T, rows_total, S);
    DH_LAUNCH_CHECK();
}
