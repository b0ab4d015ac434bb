// Token sampler: Gumbel-max sampling at temperature
// tau (greedy argmax when tau <= 0) fused with the decode bookkeeping.
//
// sample:  grid (segments, B).  Each workgroup scans one vocabulary segment
//          of row b (16-B bf16 loads), adds Gumbel noise
//          g = -log(-log(u)), u = hash(seed_b, position_b, token) -- a
//          counter-based hash, so a sequence's samples do not depend on how
//          it was batched -- and folds (value, token) into one 64-bit key
//          (order-preserving float bits << 32 | ~token: ties -> lowest id)
//          that is atomicMax'ed into result[b].  Equivalent to sampling from
//          softmax(logits / tau) without a softmax or a sort.
// finish:  one lane per row: decode the winner, reset result[b] to 0 for
//          the next launch, append the token to out_tokens, feed it as the
//          next input id, advance the position, and retire the row on EOS or
//          max_new.  The stop ids are read from device memory at EVERY launch
//          (EOS_SLOTS ints, -1 = unused slot), never passed by value: a
//          captured decode graph then follows whatever stop set the engine
//          holds when it is replayed (generate(ignore_eos=True) writes -1s),
//          not the one it held when the graph was captured.  A retired row keeps its position, so a captured decode
//          graph can keep running it harmlessly until the host drops it.
// filter:  top-k / top-p (ops/reference.py nucleus_threshold is the definition).  bf16 logits have at
//          most 65536 distinct values, so a per-row integer histogram over the 16-bit order-preserving
//          key gives the cut exactly, without a sort or a softmax pass:
//          filter_hist   grid (FILTER_R, B): workgroup (r, b) counts the keys [r, r + 1) * 65536 / R of
//                        row b in LDS (u32, LDS atomics) and stores its slice of hist[b] with plain 16-B
//                        stores, with the total of every 64-bin chunk -- no global atomics;
//          filter_select one workgroup per row walks the bins from the top: integer counts for top-k,
//                        fp32 mass n * exp((v - v1) / tau) for top-p (a fixed order: 64 bins per thread,
//                        then a block scan -- no float atomics), and writes thresh[b] (-inf: no filter);
//          sample_kernel<true> then skips every token with logit < thresh[b].  Rows without a filter
//          (or greedy, or done) cost one early-exit workgroup each and sample exactly as unfiltered.
// Tensor parallel (vocab-parallel LM head): each rank scans its vocab shard with
// tok_offset = rank * V_local -- the noise is a function of the GLOBAL token id, so the
// per-rank winners max-reduced across ranks (8 bytes per row, parallel/custom_ar.py) give the
// same token as one GPU scanning the whole row, without gathering the logits.
#include "common.h"

constexpr int EOS_SLOTS = 4;  // engine DecodeState.eos: 4 device ints, -1 = unused

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ unsigned int order_key(float v) {
    const unsigned int b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ------------------------------------------------------------------ top-k / top-p filter
constexpr int FILTER_BINS = 65536;                 // one per bf16 bit pattern
constexpr int FILTER_R = 4;                        // histogram workgroups per row
constexpr int FILTER_SLICE = FILTER_BINS / FILTER_R;  // 16384 u32 bins = 64 KiB of LDS
constexpr int HIST_THREADS = 1024;
constexpr int SELECT_THREADS = 1024;
constexpr int SELECT_CHUNK = FILTER_BINS / SELECT_THREADS;  // 64 bins per thread
// a row of the workspace: the 65536 bins, then the total count of every 64-bin chunk (the select kernel
// reads the bins of non-empty chunks only: a row of logits populates a few percent of them)
constexpr int FILTER_CHUNKS = FILTER_BINS / SELECT_CHUNK;
constexpr int FILTER_ROW = FILTER_BINS + FILTER_CHUNKS;

// order_key on the 16 bits of a bf16, -0 canonicalised to +0; NaNs -> -1 (no bin)
__device__ __forceinline__ int key16(unsigned int h) {
    if ((h & 0x7fffu) > 0x7f80u) return -1;
    if (h == 0x8000u) h = 0u;
    return (int)((h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u));
}

__device__ __forceinline__ float key16_value(int key) {
    const unsigned int h = key >= 0x8000 ? ((unsigned int)key & 0x7fffu) : (~(unsigned int)key & 0xffffu);
    return bf16_bits_to_f32(h);
}

// exp((v - v1) / tau) of the level with this key; exactly 1 for the top level (also when v1 is infinite)
__device__ __forceinline__ float level_weight(int key, int top_key, float v1, float inv_tau) {
    return key == top_key ? 1.f : __expf((key16_value(key) - v1) * inv_tau);
}

__device__ __forceinline__ bool filter_active(float tau, int k, float p) { return tau > 0.f && (k > 0 || p < 1.f); }

__global__ __launch_bounds__(HIST_THREADS) void filter_hist_kernel(const bf16* __restrict__ logits, int ld, int V,
                                                                   const float* __restrict__ temps,
                                                                   const int* __restrict__ top_k,
                                                                   const float* __restrict__ top_p,
                                                                   const int* __restrict__ done,
                                                                   unsigned int* __restrict__ hist) {
    __shared__ unsigned int bins[FILTER_SLICE];
    const int b = blockIdx.y;
    if (!filter_active(temps[b], top_k[b], top_p[b]) || done[b]) return;  // block-uniform
    const int k0 = blockIdx.x * FILTER_SLICE;
    uint4* bins4 = reinterpret_cast<uint4*>(bins);
    for (int i = threadIdx.x; i < FILTER_SLICE / 4; i += HIST_THREADS) bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const bf16* row = logits + (size_t)b * ld;
    const unsigned short* rbits = reinterpret_cast<const unsigned short*>(row);
    for (int c = threadIdx.x * 8; c < V; c += HIST_THREADS * 8) {
        unsigned int h[8];
        if (c + 8 <= V) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + c);
            h[0] = v.x & 0xffffu; h[1] = v.x >> 16; h[2] = v.y & 0xffffu; h[3] = v.y >> 16;
            h[4] = v.z & 0xffffu; h[5] = v.z >> 16; h[6] = v.w & 0xffffu; h[7] = v.w >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = c + j < V ? (unsigned int)rbits[c + j] : 0x7fffu;  // NaN: no bin
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned int rel = (unsigned int)(key16(h[j]) - k0);  // key -1 (NaN) wraps out of range
            if (rel < (unsigned int)FILTER_SLICE) atomicAdd(&bins[rel], 1u);
        }
    }
    __syncthreads();
    unsigned int* hrow = hist + (size_t)b * FILTER_ROW;
    uint4* out4 = reinterpret_cast<uint4*>(hrow + k0);
    for (int i = threadIdx.x; i < FILTER_SLICE / 4; i += HIST_THREADS) out4[i] = bins4[i];
    if (threadIdx.x < FILTER_SLICE / SELECT_CHUNK) {  // this slice's chunk totals (lane-rotated: no bank conflict)
        unsigned int t = 0;
#pragma unroll 8
        for (int i = 0; i < SELECT_CHUNK; ++i)
            t += bins[threadIdx.x * SELECT_CHUNK + ((i + threadIdx.x) & (SELECT_CHUNK - 1))];
        hrow[FILTER_BINS + k0 / SELECT_CHUNK + threadIdx.x] = t;
    }
}

// Exclusive prefix of (count, mass) over the block's threads in thread order (thread 0 = the top chunk):
// wave inclusive scan, then the earlier waves' totals added one after the other -- a fixed order.
__device__ __forceinline__ void select_scan(int cnt, float mass, int* s_cnt, float* s_mass, int& ex_cnt,
                                            float& ex_mass, int& tot_cnt) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int ic = cnt;
    float im = mass;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int oc = __shfl_up(ic, o, 64);
        const float om = __shfl_up(im, o, 64);
        if (lane >= o) { ic += oc; im = om + im; }
    }
    if (lane == 63) { s_cnt[wid] = ic; s_mass[wid] = im; }
    __syncthreads();
    int pc = 0, tc = 0;
    float pm = 0.f;
    for (int w = 0; w < SELECT_THREADS / 64; ++w) {
        if (w < wid) { pc += s_cnt[w]; pm += s_mass[w]; }
        tc += s_cnt[w];
    }
    const float prev = __shfl_up(im, 1, 64);
    ex_cnt = pc + ic - cnt;
    ex_mass = lane == 0 ? pm : pm + prev;
    tot_cnt = tc;
    __syncthreads();
}

__device__ __forceinline__ int block_max_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = red[0];
    for (int w = 1; w < SELECT_THREADS / 64; ++w) m = max(m, red[w]);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(SELECT_THREADS) void filter_select_kernel(const unsigned int* __restrict__ hist, int V,
                                                                       const float* __restrict__ temps,
                                                                       const int* __restrict__ top_k,
                                                                       const float* __restrict__ top_p,
                                                                       const int* __restrict__ done,
                                                                       float* __restrict__ thresh) {
    __shared__ int s_cnt[SELECT_THREADS / 64];
    __shared__ float s_mass[SELECT_THREADS / 64];
    __shared__ int s_red[SELECT_THREADS / 64];
    __shared__ int s_jk;
    __shared__ float s_z;
    const int b = blockIdx.x;
    const float tau = temps[b];
    const int k = top_k[b];
    const float p = top_p[b];
    if (!filter_active(tau, k, p) || done[b]) {  // block-uniform
        if (threadIdx.x == 0) thresh[b] = -INFINITY;
        return;
    }
    // thread t owns the keys hi, hi - 1, ..., hi - 63 (descending: thread 0 holds the largest values);
    // n[i] = count of key lo + i
    const int lo = FILTER_BINS - SELECT_CHUNK * ((int)threadIdx.x + 1);
    unsigned int n[SELECT_CHUNK];
    const unsigned int* hrow = hist + (size_t)b * FILTER_ROW;
    const uint4* src = reinterpret_cast<const uint4*>(hrow + lo);
    const bool any = hrow[FILTER_BINS + lo / SELECT_CHUNK] != 0u;  // coalesced; most chunks are empty
#pragma unroll
    for (int i = 0; i < SELECT_CHUNK / 4; ++i) {
        const uint4 v = any ? src[i] : make_uint4(0u, 0u, 0u, 0u);
        n[4 * i] = v.x; n[4 * i + 1] = v.y; n[4 * i + 2] = v.z; n[4 * i + 3] = v.w;
    }
    int cnt = 0, top = -1;
#pragma unroll
    for (int i = 0; i < SELECT_CHUNK; ++i) {
        cnt += (int)n[i];
        if (n[i]) top = lo + i;
    }
    const int top_key = block_max_int(top, s_red);
    if (top_key < 0) {  // nothing but NaNs
        if (threadIdx.x == 0) thresh[b] = -INFINITY;
        return;
    }
    const float v1 = key16_value(top_key);
    const float inv_tau = 1.f / tau;
    // level weights n * exp((v - v1) / tau), summed downwards within the chunk
    float mass = 0.f;
#pragma unroll
    for (int i = SELECT_CHUNK - 1; i >= 0; --i) {
        const int key = lo + i;
        if (n[i]) mass += (float)n[i] * level_weight(key, top_key, v1, inv_tau);
    }
    int ex_cnt, tot;
    float ex_mass;
    select_scan(cnt, mass, s_cnt, s_mass, ex_cnt, ex_mass, tot);
    // top-k: the first level whose cumulative count reaches k (all levels for k = 0 or k >= V)
    const int k_eff = (k <= 0 || k >= V) ? tot : min(k, tot);
    if (ex_cnt < k_eff && k_eff <= ex_cnt + cnt) {  // exactly one thread
        int c = ex_cnt, jk = -1;
        float m = ex_mass, z = 0.f;
#pragma unroll
        for (int i = SELECT_CHUNK - 1; i >= 0; --i) {
            const int key = lo + i;
            if (n[i] && jk < 0) {
                c += (int)n[i];
                m += (float)n[i] * level_weight(key, top_key, v1, inv_tau);
                if (c >= k_eff) { jk = key; z = m; }
            }
        }
        s_jk = jk;
        s_z = z;
    }
    __syncthreads();
    const int jk = s_jk;
    int cut = jk;
    if (p < 1.f) {
        // top-p over the top-k set: the first level whose cumulative mass reaches p * Z
        const float target = p * s_z;
        int cand = -1;
        float m = ex_mass;
#pragma unroll
        for (int i = SELECT_CHUNK - 1; i >= 0; --i) {
            const int key = lo + i;
            if (n[i] && key >= jk && cand < 0) {
                m += (float)n[i] * level_weight(key, top_key, v1, inv_tau);
                if (m >= target) cand = key;
            }
        }
        cand = block_max_int(cand, s_red);
        if (cand >= 0) cut = cand;
    }
    if (threadIdx.x == 0) thresh[b] = key16_value(cut);
}

// ------------------------------------------------------------------ repetition / frequency / presence penalties
// penalize: one workgroup per row rewrites, in place and before the sampler (and the filter) runs, the logits
//          of the tokens the row has generated so far (ops/reference.py apply_penalties is the definition):
//          x = rep > 0 ? x / rep : x * rep;  x -= freq * count;  x -= pres;  every step one rounded fp32
//          operation, stored back as bf16 (RNE).  The counts are a function of out_tokens[b, :gen_count[b]]
//          alone, rebuilt at every launch: the tokens are reduced to (distinct token, count) in an LDS
//          open-addressing table (LDS atomics; 2 slots per token at least, multiplicative hash, linear
//          probing), then every occupied slot rewrites its token's logit -- one thread per distinct token, no
//          global atomics, no workspace.  A neutral, done or empty row costs one early-exit workgroup.
//          TABLE = false is the other form of the same reduction, an ownership scan over the staged tokens
//          (the thread holding a token's first occurrence counts the others): O(gen_count^2 / threads) LDS
//          reads, kept for the measurement in tools/bench_sampler.py (profiles/sampler_penalties.jsonl).
constexpr int PEN_THREADS = 512;
constexpr int PEN_CAP = 4096;            // most generated tokens per row (ops.hip.PENALTY_MAX_TOKENS)
constexpr int PEN_SLOTS = 2 * PEN_CAP;   // 2 x 32 KiB of LDS: keys + counts

__device__ __forceinline__ void penalize_logit(bf16* p, int count, float rep, float freq, float pres) {
    // The reference rounds every step, so no product may be fused into the subtraction after it.  The
    // library is built with -ffp-contract=fast, under which the backend fuses whatever the pragma says:
    // the empty asm statements make the two products opaque to it.
#pragma clang fp contract(off)
    float x = (float)*p;
    if (rep != 1.f) x = x > 0.f ? x / rep : x * rep;
    float f = freq * (float)count;
    asm volatile("" : "+v"(x), "+v"(f));
    x = x - f;
    x = x - pres;
    *p = (bf16)x;
}

template <bool TABLE>
__global__ __launch_bounds__(PEN_THREADS) void penalize_kernel(bf16* __restrict__ logits, int ld, int V,
                                                               int tok_offset, const int* __restrict__ out_tokens,
                                                               int out_stride, const int* __restrict__ gen_count,
                                                               const int* __restrict__ done,
                                                               const float* __restrict__ rep_pen,
                                                               const float* __restrict__ freq_pen,
                                                               const float* __restrict__ pres_pen) {
    __shared__ int s_key[PEN_SLOTS];
    __shared__ int s_cnt[PEN_SLOTS];
    const int b = blockIdx.x;
    const float rep = rep_pen[b], freq = freq_pen[b], pres = pres_pen[b];
    const int g = min(min(gen_count[b], out_stride), PEN_CAP);  // (the launcher refuses wider token rows)
    if ((rep == 1.f && freq == 0.f && pres == 0.f) || g <= 0 || (done != nullptr && done[b])) return;  // block-uniform
    const int* toks = out_tokens + (size_t)b * out_stride;
    bf16* row = logits + (size_t)b * ld;
    if constexpr (TABLE) {
        int lg = 32 - __clz(2 * g - 1);  // slots = 2^lg >= 2 g: the probe of an absent key always ends
        lg = max(lg, 6);
        const int slots = 1 << lg;
        for (int i = threadIdx.x; i < slots; i += PEN_THREADS) { s_key[i] = -1; s_cnt[i] = 0; }
        __syncthreads();
        for (int i = threadIdx.x; i < g; i += PEN_THREADS) {
            const int t = toks[i];
            if ((unsigned int)t - (unsigned int)tok_offset >= (unsigned int)V) continue;  // another shard's token
            unsigned int h = ((unsigned int)t * 2654435761u) >> (32 - lg);
            for (;;) {
                const int prev = atomicCAS(&s_key[h], -1, t);
                if (prev == -1 || prev == t) break;
                h = (h + 1) & (unsigned int)(slots - 1);
            }
            atomicAdd(&s_cnt[h], 1);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += PEN_THREADS) {
            const int t = s_key[i];
            if (t >= 0) penalize_logit(row + (t - tok_offset), s_cnt[i], rep, freq, pres);
        }
    } else {
        for (int i = threadIdx.x; i < g; i += PEN_THREADS) s_key[i] = toks[i];
        __syncthreads();
        for (int i = threadIdx.x; i < g; i += PEN_THREADS) {
            const int t = s_key[i];
            if ((unsigned int)t - (unsigned int)tok_offset >= (unsigned int)V) continue;
            int c = 0;
            bool first = true;
            for (int j = 0; j < g; ++j) {
                const bool same = s_key[j] == t;
                c += same;
                first = first && !(same && j < i);
            }
            if (first) penalize_logit(row + (t - tok_offset), c, rep, freq, pres);
        }
    }
}

// ------------------------------------------------------------------ logit bias / minimum length / row stop ids
// constrain: one workgroup per row rewrites, in place and before the penalties, the filter and the sampler
//          run, the logits a request constrains (ops/reference.py apply_constraints is the definition):
//          entry i < bias_n[b] of the row's (bias_tok, bias_val) list -- one thread per entry, the tokens of
//          a row are distinct -- becomes bf16(float(x) + bias), one rounded fp32 add, or -inf when the bias is
//          -inf (a ban: stored, not added, so a +inf logit is banned too and no NaN appears; a NaN logit
//          stays a NaN).  Then, after a barrier (suppression wins over a bias on the same token), a row with
//          gen_count[b] < min_new[b] gets -inf at every armed stop id: the engine's EOS_SLOTS ids and the
//          row's STOP_SLOTS own ones, both read from device memory at EVERY launch (-1 = unused slot), so a
//          captured graph follows generate(ignore_eos=True) at replay.  Columns are shard-local (tok_offset /
//          V, as in penalize).  No global atomics, no workspace; a neutral or done row costs one early-exit
//          workgroup.
constexpr int CON_THREADS = 320;  // 5 waves: one pass over the 300 entries a row may hold (OpenAI's limit)
constexpr int STOP_SLOTS = 4;     // engine DecodeState.stop_ids: 4 device ints per row, -1 = unused

__global__ __launch_bounds__(CON_THREADS) void constrain_kernel(bf16* __restrict__ logits, int ld, int V,
                                                                int tok_offset, const int* __restrict__ bias_tok,
                                                                const float* __restrict__ bias_val, int bias_stride,
                                                                const int* __restrict__ bias_n,
                                                                const int* __restrict__ gen_count,
                                                                const int* __restrict__ min_new,
                                                                const int* __restrict__ stop_ids,
                                                                const int* __restrict__ eos,
                                                                const int* __restrict__ done) {
    const int b = blockIdx.x;
    const int n = min(bias_n[b], bias_stride);
    const bool suppress = gen_count[b] < min_new[b];
    if ((n <= 0 && !suppress) || (done != nullptr && done[b])) return;  // block-uniform
    bf16* row = logits + (size_t)b * ld;
    unsigned short* rbits = reinterpret_cast<unsigned short*>(row);
    for (int i = threadIdx.x; i < n; i += CON_THREADS) {
        const unsigned int col = (unsigned int)bias_tok[(size_t)b * bias_stride + i] - (unsigned int)tok_offset;
        if (col >= (unsigned int)V) continue;  // another shard's token
        const float bias = bias_val[(size_t)b * bias_stride + i];
        const float x = (float)row[col];
        if (bias != -INFINITY) row[col] = (bf16)(x + bias);
        else if (x == x) rbits[col] = 0xff80u;  // -inf
    }
    if (!suppress) return;  // block-uniform
    __syncthreads();  // the biased logits are written: a suppressed stop id overwrites its bias
    if (threadIdx.x < EOS_SLOTS + STOP_SLOTS) {
        const int t = threadIdx.x < EOS_SLOTS ? eos[threadIdx.x]
                                              : stop_ids[(size_t)b * STOP_SLOTS + (threadIdx.x - EOS_SLOTS)];
        const unsigned int col = (unsigned int)t - (unsigned int)tok_offset;
        if (t >= 0 && col < (unsigned int)V) rbits[col] = 0xff80u;
    }
}

template <bool FILTER>
__global__ __launch_bounds__(256) void sample_kernel(const bf16* __restrict__ logits, int ld, int V, int tok_offset,
                                                     const float* __restrict__ temps,
                                                     const long long* __restrict__ seeds,
                                                     const int* __restrict__ positions,
                                                     unsigned long long* __restrict__ result, int seg_len,
                                                     const float* __restrict__ thresh) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.y;
    const float tau = temps[b];
    float th = -INFINITY;
    if constexpr (FILTER) th = thresh[b];
    const float inv_tau = tau > 0.f ? 1.f / tau : 0.f;
    const unsigned long long key0 =
        mix64((unsigned long long)seeds[b] * 0x9E3779B97F4A7C15ULL + (unsigned long long)(positions[b] + 1));
    const int c0 = blockIdx.x * seg_len;
    const int c1 = min(V, c0 + seg_len);
    const bf16* row = logits + (size_t)b * ld;
    unsigned long long best = 0;
    for (int c = c0 + threadIdx.x * 8; c < c1; c += 256 * 8) {
        float f[8];
        if (c + 8 <= c1) {
            unpack8(*reinterpret_cast<const uint4*>(row + c), f);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = c + j < c1 ? (float)row[c + j] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int tok = tok_offset + c + j;
            float v = f[j];
            if constexpr (FILTER) {
                if (v < th) continue;  // outside the kept set: no hash, no key
            }
            if (tau > 0.f) {
                const unsigned long long h = mix64(key0 ^ ((unsigned long long)tok * 0xD1B54A32D192ED03ULL));
                const float u = ((float)(h >> 40) + 0.5f) * (1.f / 16777216.f);
                v = v * inv_tau - __logf(-__logf(u));
            }
            const unsigned long long k =
                ((unsigned long long)order_key(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)tok);
            if (c + j < c1 && k > best) best = k;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = red[0];
        for (int i = 1; i < 4; ++i) m = red[i] > m ? red[i] : m;
        atomicMax(result + b, m);
    }
}

// ROW_STOPS: the row's own STOP_SLOTS stop ids (stop_ids[b], -1 = unused) retire it like an EOS id, the
// token appended as an EOS id is.  ROW_STOPS = false never touches stop_ids: the plain finish, instruction
// for instruction the kernel it was before the row stops existed.
template <bool ROW_STOPS>
__device__ __forceinline__ void finish_row(unsigned long long* __restrict__ result, int* __restrict__ next_ids,
                                           int* __restrict__ positions, int* __restrict__ gen_count,
                                           const int* __restrict__ max_new, int* __restrict__ out_tokens,
                                           int out_stride, int* __restrict__ done, const int* __restrict__ eos,
                                           const int* __restrict__ stop_ids, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long r = result[b];
    result[b] = 0ULL;
    if (done[b]) return;
    const int tok = (int)(0xFFFFFFFFu - (unsigned int)(r & 0xFFFFFFFFULL));
    const int g = gen_count[b];
    out_tokens[(size_t)b * out_stride + g] = tok;
    gen_count[b] = g + 1;
    next_ids[b] = tok;
    bool stop = g + 1 >= max_new[b];
#pragma unroll
    for (int i = 0; i < EOS_SLOTS; ++i) stop |= tok == eos[i];  // tok >= 0 never matches a -1 slot
    if constexpr (ROW_STOPS) {
        const int4 own = *reinterpret_cast<const int4*>(stop_ids + (size_t)b * STOP_SLOTS);  // 16-B aligned rows
        stop |= tok == own.x || tok == own.y || tok == own.z || tok == own.w;
    }
    if (stop) done[b] = 1;
    else positions[b] += 1;
}

__global__ void sample_finish_kernel(unsigned long long* __restrict__ result, int* __restrict__ next_ids,
                                     int* __restrict__ positions, int* __restrict__ gen_count,
                                     const int* __restrict__ max_new, int* __restrict__ out_tokens, int out_stride,
                                     int* __restrict__ done, const int* __restrict__ eos, int B) {
    finish_row<false>(result, next_ids, positions, gen_count, max_new, out_tokens, out_stride, done, eos, nullptr, B);
}

__global__ void sample_finish_stops_kernel(unsigned long long* __restrict__ result, int* __restrict__ next_ids,
                                           int* __restrict__ positions, int* __restrict__ gen_count,
                                           const int* __restrict__ max_new, int* __restrict__ out_tokens,
                                           int out_stride, int* __restrict__ done, const int* __restrict__ eos,
                                           const int* __restrict__ stop_ids, int B) {
    finish_row<true>(result, next_ids, positions, gen_count, max_new, out_tokens, out_stride, done, eos, stop_ids, B);
}

// ------------------------------------------------------------------ token log-probabilities
// logprobs: the log-softmax of the rows the sampler is about to see (after constrain / penalize, at T = 1, before
//          the filter) and their top lists (ops/reference.py token_logprobs is the definition).  The kernels
//          only read the logits.
//          logprobs_seg   grid (LP_SEGS, B): workgroup (s, b) scans segment s of row b (16-B loads, scalar tail)
//                         once per quantity -- its largest key, its sum exp(x - segment max), then, every wave
//                         on its own columns and without a barrier, one pass per top entry (the largest key
//                         below the previous one: the keys of a row are distinct, (order key of the value, -0
//                         as +0) << 32 | ~token, so ties go to the lower id); wave 0 picks the segment's n
//                         largest of the four lists.  A thread keeps the keys of its first 16 columns in
//                         registers -- a whole segment up to V = 131072, so a Llama-3 row is read once --
//                         and reads the columns past them again in every pass (this CU's L1 / the L2), so no
//                         V is too large.  It stores (max, sum) and its lp_n[b] keys with plain stores into
//                         the row's workspace.
//          logprobs_merge one wave per row, a second kernel: the kernel boundary makes the segments' plain
//                         stores visible, where a last-arriver tail would need a ticket atomic, its reset and
//                         fences for a merge this small.  It folds the segments IN SEGMENT ORDER -- M = max,
//                         S = sum_s sum_s * exp(max_s - M), one thread adding the 32 terms one after the other
//                         -- picks the top lp_n[b] of the <= 32 * lp_n[b] keys and writes them with
//                         lp = (v - M) - log S straight into the row's record of step gen_count[b], read
//                         BEFORE the finish advances it.  lse_m / lse_logS / lp_slot hand M, log S and that
//                         step to the pick kernel; lp_slot[b] = -1 says "no record this step".
//          logprobs_pick  after the finish (whichever ran): one thread per row with lp_slot[b] >= 0 reads the
//                         token the finish appended and its logit from the still unmodified row and stores
//                         (v - M) - log S, the very operations of the top list: bit-equal to its entry there.
//          Rows with lp_n[b] < 0 (off), done rows and rows whose step is past the record width write no
//          record; their lp_slot is -1, so the pick skips them (a done row keeps running in a captured graph:
//          a stale slot would rewrite its last record from the wrong logits).  No global atomics, no float
//          atomics, nothing depends on B or on the row's index: the same row gives the same bits anywhere.
constexpr int LP_SEGS = 32;
constexpr int LP_TOP = 20;  // OpenAI's top_logprobs limit (ops.hip.LOGPROBS_TOP)
constexpr int LP_THREADS = 256;
constexpr int LP_MERGE_KEYS = LP_SEGS * LP_TOP / 64;  // keys per lane of the merging wave
constexpr int LP_CACHE = 2;  // 16-B loads of a thread whose keys stay in registers (32 VGPRs)
constexpr int LP_WAVE_KEYS = ((LP_THREADS / 64) * LP_TOP + 63) / 64;  // ... and of a segment's wave 0

__device__ __forceinline__ unsigned long long lp_key(float v, int tok) {
    unsigned int bits = __float_as_uint(v);
    if (bits == 0x80000000u) bits = 0u;  // -0 -> +0: compared as numbers
    const unsigned int o = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)tok);
}

__device__ __forceinline__ float lp_key_value(unsigned long long k) {
    const unsigned int o = (unsigned int)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ unsigned long long lp_wave_max(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o, 64);
        k = other > k ? other : k;
    }
    return k;
}

__device__ __forceinline__ unsigned long long lp_block_max(unsigned long long k, unsigned long long* red) {
    k = lp_wave_max(k);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    unsigned long long m = red[0];
    for (int i = 1; i < LP_THREADS / 64; ++i) m = red[i] > m ? red[i] : m;
    __syncthreads();
    return m;
}

// f(value, column) over this thread's share of the columns [c0, c1) of a row (c0 a multiple of 8)
template <class F>
__device__ __forceinline__ void lp_scan(const bf16* __restrict__ row, int c0, int c1, F f) {
    for (int c = c0 + threadIdx.x * 8; c < c1; c += LP_THREADS * 8) {
        float x[8];
        if (c + 8 <= c1) {
            unpack8(*reinterpret_cast<const uint4*>(row + c), x);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = c + j < c1 ? (float)row[c + j] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c + j < c1) f(x[j], c + j);
    }
}

__device__ __forceinline__ bool lp_row_live(int n, int g, int done, int cap) { return n >= 0 && !done && g < cap; }

__global__ __launch_bounds__(LP_THREADS) void logprobs_seg_kernel(const bf16* __restrict__ logits, int ld, int V,
                                                                  const int* __restrict__ lp_n,
                                                                  const int* __restrict__ gen_count,
                                                                  const int* __restrict__ done, int cap, int seg_len,
                                                                  float2* __restrict__ seg_ms,
                                                                  unsigned long long* __restrict__ seg_keys) {
    __shared__ unsigned long long red[LP_THREADS / 64];
    __shared__ float fred[LP_THREADS / 64];
    __shared__ unsigned long long s_keys[LP_THREADS / 64][LP_TOP];
    const int b = blockIdx.y;
    const int n = min(lp_n[b], LP_TOP);
    if (!lp_row_live(n, gen_count[b], done[b], cap)) return;  // block-uniform
    const int c0 = min(V, (int)blockIdx.x * seg_len);  // (a short row leaves its last segments empty)
    const int c1 = min(V, c0 + seg_len);
    const bf16* row = logits + (size_t)b * ld;
    // the keys of this thread's first LP_CACHE x 8 columns stay in registers (a whole segment up to V = 32 *
    // LP_CACHE * 2048 = 131072); the columns past them are read again in every pass, from this CU's L1 / the L2
    unsigned long long kc[LP_CACHE * 8];  // 0 = no column: no key is 0, a token id is below 2^31
#pragma unroll
    for (int i = 0; i < LP_CACHE; ++i) {
        const int c = c0 + (i * LP_THREADS + (int)threadIdx.x) * 8;
        float x[8];
        if (c + 8 <= c1) {
            unpack8(*reinterpret_cast<const uint4*>(row + c), x);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = c + j < c1 ? (float)row[c + j] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) kc[i * 8 + j] = c + j < c1 ? lp_key(x[j], c + j) : 0ULL;
    }
    const int cr = min(c1, c0 + LP_CACHE * LP_THREADS * 8);  // [cr, c1): the columns not cached
    unsigned long long best = 0ULL;
#pragma unroll
    for (int i = 0; i < LP_CACHE * 8; ++i) best = kc[i] > best ? kc[i] : best;
    lp_scan(row, cr, c1, [&](float v, int t) {
        const unsigned long long k = lp_key(v, t);
        best = k > best ? k : best;
    });
    best = lp_block_max(best, red);
    const float m = best ? lp_key_value(best) : -INFINITY;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LP_CACHE * 8; ++i) {
        const float v = lp_key_value(kc[i]);  // (-0 comes back as +0: the same exp)
        s += (kc[i] && v > -INFINITY) ? __expf(v - m) : 0.f;
    }
    lp_scan(row, cr, c1, [&](float v, int) { s += v > -INFINITY ? __expf(v - m) : 0.f; });
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) fred[threadIdx.x >> 6] = s;
    __syncthreads();
    const size_t seg = (size_t)b * LP_SEGS + blockIdx.x;
    if (threadIdx.x == 0) {
        float t = fred[0];
        for (int i = 1; i < LP_THREADS / 64; ++i) t += fred[i];
        seg_ms[seg] = make_float2(m, t);
    }
    if (n == 0) return;  // block-uniform
    // the top n: every wave lists the n largest keys of its own columns (one pass over its keys and one wave
    // reduction per entry, no barrier), then wave 0 picks the n largest of the LP_THREADS / 64 lists
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long prev = ~0ULL;
    for (int r = 0; r < n; ++r) {  // wave-uniform
        unsigned long long next = 0ULL;
        if (prev) {
#pragma unroll
            for (int i = 0; i < LP_CACHE * 8; ++i) next = (kc[i] < prev && kc[i] > next) ? kc[i] : next;
            lp_scan(row, cr, c1, [&](float v, int t) {
                const unsigned long long k = lp_key(v, t);
                next = (k < prev && k > next) ? k : next;
            });
            next = lp_wave_max(next);
        }
        if (lane == 0) s_keys[wid][r] = next;  // 0 once the wave's columns are exhausted
        prev = next;
    }
    __syncthreads();
    if (wid != 0) return;
    unsigned long long k[LP_WAVE_KEYS];
#pragma unroll
    for (int j = 0; j < LP_WAVE_KEYS; ++j) {
        const int i = lane + 64 * j;  // list i / LP_TOP, entry i % LP_TOP
        k[j] = (i < (LP_THREADS / 64) * LP_TOP && i % LP_TOP < n) ? s_keys[i / LP_TOP][i % LP_TOP] : 0ULL;
    }
    unsigned long long* keys = seg_keys + seg * LP_TOP;
    prev = ~0ULL;
    for (int r = 0; r < n; ++r) {
        unsigned long long next = 0ULL;
#pragma unroll
        for (int j = 0; j < LP_WAVE_KEYS; ++j) next = (k[j] < prev && k[j] > next) ? k[j] : next;
        next = lp_wave_max(next);
        if (lane == 0) keys[r] = next;  // 0 once the segment is exhausted
        prev = next;
    }
}

__global__ __launch_bounds__(64) void logprobs_merge_kernel(const int* __restrict__ lp_n,
                                                            const int* __restrict__ gen_count,
                                                            const int* __restrict__ done, int cap,
                                                            const float2* __restrict__ seg_ms,
                                                            const unsigned long long* __restrict__ seg_keys,
                                                            float* __restrict__ lse_m, float* __restrict__ lse_logS,
                                                            int* __restrict__ lp_slot, int* __restrict__ out_top_tok,
                                                            float* __restrict__ out_top_lp) {
    __shared__ float s_term[LP_SEGS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(lp_n[b], LP_TOP);
    const int g = gen_count[b];
    if (!lp_row_live(n, g, done[b], cap)) {  // block-uniform
        if (lane == 0) lp_slot[b] = -1;
        return;
    }
    const float2 ms = lane < LP_SEGS ? seg_ms[(size_t)b * LP_SEGS + lane] : make_float2(-INFINITY, 0.f);
    const float M = wave_max(ms.x);
    if (lane < LP_SEGS) s_term[lane] = ms.x > -INFINITY ? ms.y * __expf(ms.x - M) : 0.f;
    __syncthreads();
    float S = 0.f;
    for (int i = 0; i < LP_SEGS; ++i) S += s_term[i];  // segment order, the same on every lane
    const float logS = __logf(S);
    unsigned long long k[LP_MERGE_KEYS];
    const unsigned long long* keys = seg_keys + (size_t)b * (LP_SEGS * LP_TOP);
#pragma unroll
    for (int j = 0; j < LP_MERGE_KEYS; ++j) {
        const int i = lane + 64 * j;
        k[j] = i % LP_TOP < n ? keys[i] : 0ULL;  // a segment wrote its first n slots only
    }
    unsigned long long prev = ~0ULL;
    int my_tok = -1;
    float my_lp = -INFINITY;
    for (int r = 0; r < n; ++r) {
        unsigned long long best = 0ULL;
#pragma unroll
        for (int j = 0; j < LP_MERGE_KEYS; ++j) best = (k[j] < prev && k[j] > best) ? k[j] : best;
        best = lp_wave_max(best);
        if (lane == r && best) {  // (fewer than n tokens in the row: the other entries stay -1 / -inf)
            my_tok = (int)(0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFULL));
            my_lp = (lp_key_value(best) - M) - logS;
        }
        prev = best;
    }
    if (lane < n) {
        const size_t at = ((size_t)b * cap + g) * LP_TOP + lane;
        out_top_tok[at] = my_tok;
        out_top_lp[at] = my_lp;
    }
    if (lane == 0) {
        lse_m[b] = M;
        lse_logS[b] = logS;
        lp_slot[b] = g;
    }
}

__global__ void logprobs_pick_kernel(const bf16* __restrict__ logits, int ld, int V,
                                     const int* __restrict__ out_tokens, int out_stride,
                                     const int* __restrict__ lp_slot, const float* __restrict__ lse_m,
                                     const float* __restrict__ lse_logS, float* __restrict__ out_logprobs, int cap,
                                     int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int slot = lp_slot[b];
    if (slot < 0 || slot >= cap || slot >= out_stride) return;
    const int tok = out_tokens[(size_t)b * out_stride + slot];
    if ((unsigned int)tok >= (unsigned int)V) return;
    unsigned int bits = (unsigned int)reinterpret_cast<const unsigned short*>(logits + (size_t)b * ld)[tok] << 16;
    if (bits == 0x80000000u) bits = 0u;  // -0 -> +0, as in the top list's keys
    out_logprobs[(size_t)b * cap + slot] = (__uint_as_float(bits) - lse_m[b]) - lse_logS[b];
}

static int launch_keys(const void* logits, int ld, int B, int V, int tok_offset, const float* temps,
                       const long long* seeds, const int* positions, void* result, hipStream_t s) {
    const int nseg = 32;
    int seg_len = ceil_div(V, nseg);
    seg_len = (seg_len + 7) & ~7;
    sample_kernel<false><<<dim3(nseg, B), 256, 0, s>>>((const bf16*)logits, ld, V, tok_offset, temps, seeds,
                                                       positions, (unsigned long long*)result, seg_len, nullptr);
    return (int)hipGetLastError();
}

// Gumbel-max keys of a (shard of the) vocabulary, max-folded into result[b] (which must be 0 or an
// earlier partial key).  Tensor-parallel callers max-reduce result across ranks, then finish.
MRSUM_API int mrsum_sample_keys(const void* logits, int ld, int B, int V, int tok_offset, const float* temps,
                                const long long* seeds, const int* positions, void* result, hipStream_t s) {
    if (B <= 0) return 0;
    return launch_keys(logits, ld, B, V, tok_offset, temps, seeds, positions, result, s);
}

MRSUM_API int mrsum_sample_finish(void* result, int* next_ids, int* positions_rw, int* gen_count, const int* max_new,
                                  int* out_tokens, int out_stride, int* done, const int* eos, int B,
                                  hipStream_t s) {
    if (B <= 0) return 0;
    sample_finish_kernel<<<ceil_div(B, 64), 64, 0, s>>>((unsigned long long*)result, next_ids, positions_rw,
                                                        gen_count, max_new, out_tokens, out_stride, done, eos, B);
    return (int)hipGetLastError();
}

MRSUM_API int mrsum_sample(const void* logits, int ld, int B, int V, const float* temps, const long long* seeds,
                           const int* positions, void* result, int* next_ids, int* positions_rw, int* gen_count,
                           const int* max_new, int* out_tokens, int out_stride, int* done, const int* eos,
                           hipStream_t s) {
    if (B <= 0) return 0;
    int e = launch_keys(logits, ld, B, V, 0, temps, seeds, positions, result, s);
    if (e) return e;
    sample_finish_kernel<<<ceil_div(B, 64), 64, 0, s>>>((unsigned long long*)result, next_ids, positions_rw,
                                                        gen_count, max_new, out_tokens, out_stride, done, eos, B);
    return (int)hipGetLastError();
}

// thresh[b] = the top-k / top-p threshold of row b (-inf: no filter, greedy or done).  hist: workspace of
// B x (65536 + 1024) u32 (ops.hip.FilterWorkspace), fully rewritten for every filtered row: no state is
// carried between launches.
MRSUM_API int mrsum_sample_thresh(const void* logits, int ld, int B, int V, const float* temps, const int* top_k,
                                  const float* top_p, const int* done, float* thresh, void* hist, hipStream_t s) {
    if (B <= 0) return 0;
    filter_hist_kernel<<<dim3(FILTER_R, B), HIST_THREADS, 0, s>>>((const bf16*)logits, ld, V, temps, top_k, top_p,
                                                                  done, (unsigned int*)hist);
    int e = (int)hipGetLastError();
    if (e) return e;
    filter_select_kernel<<<B, SELECT_THREADS, 0, s>>>((const unsigned int*)hist, V, temps, top_k, top_p, done,
                                                      thresh);
    return (int)hipGetLastError();
}

// mrsum_sample with a top-k / top-p filter per row: thresholds, Gumbel-max over the kept tokens, finish --
// all on stream s, capturable.
MRSUM_API int mrsum_sample_filtered(const void* logits, int ld, int B, int V, const float* temps,
                                    const long long* seeds, const int* positions, const int* top_k,
                                    const float* top_p, float* thresh, void* hist, void* result, int* next_ids,
                                    int* positions_rw, int* gen_count, const int* max_new, int* out_tokens,
                                    int out_stride, int* done, const int* eos, hipStream_t s) {
    if (B <= 0) return 0;
    int e = mrsum_sample_thresh(logits, ld, B, V, temps, top_k, top_p, done, thresh, hist, s);
    if (e) return e;
    const int nseg = 32;
    int seg_len = ceil_div(V, nseg);
    seg_len = (seg_len + 7) & ~7;
    sample_kernel<true><<<dim3(nseg, B), 256, 0, s>>>((const bf16*)logits, ld, V, 0, temps, seeds, positions,
                                                      (unsigned long long*)result, seg_len, thresh);
    e = (int)hipGetLastError();
    if (e) return e;
    sample_finish_kernel<<<ceil_div(B, 64), 64, 0, s>>>((unsigned long long*)result, next_ids, positions_rw,
                                                        gen_count, max_new, out_tokens, out_stride, done, eos, B);
    return (int)hipGetLastError();
}

// Repetition / frequency / presence penalties on the logits rows, in place, ahead of any sampler launch on
// stream s (capturable).  V / tok_offset: the width and first global token id of the rows (a vocab-parallel
// rank's shard: tokens of other shards are skipped).  a row holds at most PEN_CAP generated tokens (the
// Python launcher refuses wider out_tokens rows).  done may be null.
MRSUM_API int mrsum_penalize(void* logits, int ld, int B, int V, int tok_offset, const int* out_tokens,
                             int out_stride, const int* gen_count, const int* done, const float* rep,
                             const float* freq, const float* pres, hipStream_t s) {
    if (B <= 0) return 0;
    penalize_kernel<true><<<B, PEN_THREADS, 0, s>>>((bf16*)logits, ld, V, tok_offset, out_tokens, out_stride,
                                                    gen_count, done, rep, freq, pres);
    return (int)hipGetLastError();
}

// The ownership-scan form of the same kernel (measurement and its equality test only).
MRSUM_API int mrsum_penalize_scan(void* logits, int ld, int B, int V, int tok_offset, const int* out_tokens,
                                  int out_stride, const int* gen_count, const int* done, const float* rep,
                                  const float* freq, const float* pres, hipStream_t s) {
    if (B <= 0) return 0;
    penalize_kernel<false><<<B, PEN_THREADS, 0, s>>>((bf16*)logits, ld, V, tok_offset, out_tokens, out_stride,
                                                     gen_count, done, rep, freq, pres);
    return (int)hipGetLastError();
}

// Logit bias, minimum length (armed stop ids at -inf while gen_count < min_new) on the logits rows, in place,
// ahead of the penalties and of any sampler launch on stream s (capturable).  bias_tok / bias_val: rows of
// bias_stride entries, the first bias_n[b] of row b valid; stop_ids: B x 4 ints; eos: the engine's 4 ints.
// V / tok_offset describe a vocabulary shard as in mrsum_penalize.  done may be null.
MRSUM_API int mrsum_constrain(void* logits, int ld, int B, int V, int tok_offset, const int* bias_tok,
                              const float* bias_val, int bias_stride, const int* bias_n, const int* gen_count,
                              const int* min_new, const int* stop_ids, const int* eos, const int* done,
                              hipStream_t s) {
    if (B <= 0) return 0;
    constrain_kernel<<<B, CON_THREADS, 0, s>>>((bf16*)logits, ld, V, tok_offset, bias_tok, bias_val, bias_stride,
                                               bias_n, gen_count, min_new, stop_ids, eos, done);
    return (int)hipGetLastError();
}

// mrsum_sample_finish that also retires a row whose new token is one of its own stop ids (stop_ids: B x 4
// ints, 16-byte aligned, -1 = unused slot).
MRSUM_API int mrsum_sample_finish_stops(void* result, int* next_ids, int* positions_rw, int* gen_count,
                                        const int* max_new, int* out_tokens, int out_stride, int* done,
                                        const int* eos, const int* stop_ids, int B, hipStream_t s) {
    if (B <= 0) return 0;
    sample_finish_stops_kernel<<<ceil_div(B, 64), 64, 0, s>>>((unsigned long long*)result, next_ids, positions_rw,
                                                              gen_count, max_new, out_tokens, out_stride, done, eos,
                                                              stop_ids, B);
    return (int)hipGetLastError();
}

// The first two stages of mrsum_sample_filtered -- thresholds, then the Gumbel-max keys over the kept tokens
// of whole rows folded into result[b] -- without the finish, so that a constrained step ends in
// mrsum_sample_finish_stops.
MRSUM_API int mrsum_sample_keys_filtered(const void* logits, int ld, int B, int V, const float* temps,
                                         const long long* seeds, const int* positions, const int* top_k,
                                         const float* top_p, const int* done, float* thresh, void* hist,
                                         void* result, hipStream_t s) {
    if (B <= 0) return 0;
    int e = mrsum_sample_thresh(logits, ld, B, V, temps, top_k, top_p, done, thresh, hist, s);
    if (e) return e;
    const int nseg = 32;
    int seg_len = ceil_div(V, nseg);
    seg_len = (seg_len + 7) & ~7;
    sample_kernel<true><<<dim3(nseg, B), 256, 0, s>>>((const bf16*)logits, ld, V, 0, temps, seeds, positions,
                                                      (unsigned long long*)result, seg_len, thresh);
    return (int)hipGetLastError();
}

// Log-probabilities of whole rows (tok_offset 0), after mrsum_constrain / mrsum_penalize and BEFORE any sampler
// launch on stream s (capturable; the logits are only read).  lp_n: -1 = off, else the row's top-list length
// 0..20.  A live row (lp_n >= 0, not done, gen_count < cap) gets its top list written into record gen_count[b]
// of out_top_tok / out_top_lp (B x cap x 20) and lse_m / lse_logS / lp_slot[b] = gen_count[b] for
// mrsum_logprobs_pick; every other row gets lp_slot[b] = -1 and nothing else.  seg_ms (B x 32 float2) and
// seg_keys (B x 32 x 20 u64) are scratch, rewritten for every live row: no state is carried between launches.
MRSUM_API int mrsum_logprobs(const void* logits, int ld, int B, int V, const int* lp_n, const int* gen_count,
                             const int* done, int cap, void* seg_ms, void* seg_keys, float* lse_m, float* lse_logS,
                             int* lp_slot, int* out_top_tok, float* out_top_lp, hipStream_t s) {
    if (B <= 0) return 0;
    int seg_len = ceil_div(V, LP_SEGS);
    seg_len = (seg_len + 7) & ~7;
    logprobs_seg_kernel<<<dim3(LP_SEGS, B), LP_THREADS, 0, s>>>((const bf16*)logits, ld, V, lp_n, gen_count, done, cap,
                                                                seg_len, (float2*)seg_ms,
                                                                (unsigned long long*)seg_keys);
    int e = (int)hipGetLastError();
    if (e) return e;
    logprobs_merge_kernel<<<B, 64, 0, s>>>(lp_n, gen_count, done, cap, (const float2*)seg_ms,
                                           (const unsigned long long*)seg_keys, lse_m, lse_logS, lp_slot, out_top_tok,
                                           out_top_lp);
    return (int)hipGetLastError();
}

// After the finish kernel (plain, row-stops, or the TP one): out_logprobs[b, lp_slot[b]] = the log-probability
// of the token the finish appended at out_tokens[b, lp_slot[b]], for every row with lp_slot[b] >= 0.
MRSUM_API int mrsum_logprobs_pick(const void* logits, int ld, int B, int V, const int* out_tokens, int out_stride,
                                  const int* lp_slot, const float* lse_m, const float* lse_logS, float* out_logprobs,
                                  int cap, hipStream_t s) {
    if (B <= 0) return 0;
    logprobs_pick_kernel<<<ceil_div(B, 64), 64, 0, s>>>((const bf16*)logits, ld, V, out_tokens, out_stride, lp_slot,
                                                        lse_m, lse_logS, out_logprobs, cap, B);
    return (int)hipGetLastError();
}
