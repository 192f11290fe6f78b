// Negative sampler on the device, bit-exact with the reference's host sampler.
//
// Replaces: recbole/sampler/sampler.py:240-241 Sampler._uni_sampling = np.random.randint(1, item_num, n), and the
// rejection loop of AbstractSampler.sample_by_key_ids (:145-197).  The third-party arithmetic underneath is numpy's
// legacy RandomState: MT19937 (mt19937_seed / mt19937_gen) and, for the int64 default dtype on a range below 2^32,
// masked rejection on single 32-bit outputs (buffered_bounded_masked_uint32).  The generator state lives in device
// memory in numpy's own layout (key[624], pos), so the stream can be handed to and taken back from
// np.random.set_state / get_state at any point.
//
// One workgroup does a whole call: the MT recurrence is sequential in blocks of 624 words (each block = four
// barrier-separated parallel phases), the accept/reject filter and the "which positions collide with the user's
// used-set" compaction are block-wide ordered scans, and the re-draw rounds loop inside the kernel until no position
// is left -- the number of rounds is data dependent, and the stream position after the call must be exact before the
// next batch draws from it, so the loop can not be cut short on the host side without a sync.
//
// Each rule is stated once: the generator in mt19937.hpp, the stream kept in LDS (MtStream), the masked-rejection draw
// (draw_bounded), the ordered compaction of the colliding positions (compact_hits) and a call's rounds (sample_call, which the
// uniform and the popularity kernel run with their own way of drawing a round).
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "mt19937.hpp"

namespace fr {

static constexpr int SAMPLER_THREADS = 1024;

// new state block from the old one (mt19937_gen's three loops as parallel phases: [0,227) reads old words only,
// [227,454) and [454,623) read words the previous phase produced, word 623 reads new[0] and new[396])
__device__ __forceinline__ void mt_twist(const uint32_t* __restrict__ o, uint32_t* __restrict__ n, int t) {
    if (t < MT_H) n[t] = mt_next_word(o, n, t);
    __syncthreads();
    if (t >= MT_H && t < 2 * MT_H) n[t] = mt_next_word(o, n, t);
    __syncthreads();
    if (t >= 2 * MT_H && t < MT_N - 1) n[t] = mt_next_word(o, n, t);
    __syncthreads();
    if (t == MT_N - 1) n[t] = mt_next_word(o, n, t);
    __syncthreads();
}

// The generator while a kernel walks it: two blocks in LDS (a twist forms the new one beside the old one), which of them is
// current, and the position of the next word in it.  `cur` and `pos` are the same in every thread of a workgroup of THREADS.
template <int THREADS>
struct MtStream {
    uint32_t (*blk)[MT_N];
    int cur, pos;
    __device__ __forceinline__ const uint32_t* block() const { return blk[cur]; }
    __device__ __forceinline__ uint32_t* other() { return blk[cur ^ 1]; }
    __device__ __forceinline__ void flip() { cur ^= 1; }
    // (a barrier between load and the first read of a word is the caller's)
    __device__ __forceinline__ void load(const uint32_t* __restrict__ state, int t) {
        for (int k = t; k < MT_N; k += THREADS) blk[0][k] = state[k];
        cur = 0;
        pos = (int)state[MT_N];
    }
    __device__ __forceinline__ void store(uint32_t* __restrict__ state, int t) const {
        for (int k = t; k < MT_N; k += THREADS) state[k] = blk[cur][k];
        if (t == 0) state[MT_N] = (uint32_t)pos;
    }
    __device__ __forceinline__ void refill(int t) {      // the next block, once the current one is used up
        static_assert(THREADS >= MT_N, "mt_twist forms one word per thread");
        if (pos == MT_N) {
            mt_twist(block(), other(), t);
            flip();
            pos = 0;
        }
    }
};
using Stream = MtStream<SAMPLER_THREADS>;

// LDS of the block-wide ordered scans
struct BlockScan {
    int wave_cnt[SAMPLER_THREADS / 64];
    int last;      // draw_bounded: the thread whose word yields the last value wanted
};

// ordered block-wide exclusive scan of one flag per thread; returns the rank, `total` = number of set flags
__device__ __forceinline__ int flag_scan(bool flag, BlockScan& sc, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();   // wave_cnt may still be read by the previous call
    if (lane == 0) sc.wave_cnt[wid] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SAMPLER_THREADS / 64; ++w) {
        const int c = sc.wave_cnt[w];
        off += w < wid ? c : 0;
        tot += c;
    }
    total = tot;
    return off + in_wave;
}

__device__ __forceinline__ bool used_contains(const int32_t* __restrict__ items, long long lo, long long hi, int v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const int x = items[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// np.random.randint(low, low + span + 1, need) from the continuing stream (span > 0): masked rejection on single words, the
// accepted values written in position order to out[list[e]] (list == nullptr: out[e])
__device__ __forceinline__ void draw_bounded(Stream& s, BlockScan& sc, long long low, uint32_t span, uint32_t mask,
                                             int64_t* __restrict__ out, const int32_t* list, long long need) {
    const int t = threadIdx.x;
    long long produced = 0;
    while (produced < need) {
        s.refill(t);
        uint32_t v = 0;
        bool acc = false;
        if (t >= s.pos && t < MT_N) {
            v = mt_temper(s.block()[t]) & mask;
            acc = v <= span;
        }
        int cnt;
        const int k = flag_scan(acc, sc, cnt);
        const long long remaining = need - produced;
        if (acc && k < remaining) {
            const long long e = produced + k;
            out[list ? (long long)list[e] : e] = low + (long long)v;
            if (k == remaining - 1) sc.last = t;     // the draw that yields the last value ends the consumption
        }
        __syncthreads();
        if (cnt >= remaining) {
            s.pos = sc.last + 1;
            produced = need;
        } else {
            s.pos = MT_N;
            produced += cnt;
        }
        __syncthreads();   // sc.last is rewritten in the next iteration
    }
}

// Which of the `need` positions just drawn (list, or [0, need)) hit?  Ordered compaction of those into `next`, the list of
// the next round; returns their number.  `hit_at(i)`: does position i collide with its key's used-set.
template <class Pred>
__device__ __forceinline__ long long compact_hits(long long need, const int32_t* list, int32_t* next, BlockScan& sc, Pred hit_at) {
    const int t = threadIdx.x;
    long long kept = 0;
    for (long long base = 0; base < need; base += SAMPLER_THREADS) {
        const long long e = base + t;
        bool hit = false;
        long long i = 0;
        if (e < need) {
            i = list ? (long long)list[e] : e;
            hit = hit_at(i);
        }
        int cnt;
        const int k = flag_scan(hit, sc, cnt);
        if (hit) next[kept + k] = (int32_t)i;
        kept += cnt;
    }
    __syncthreads();
    __threadfence_block();
    return kept;
}

struct Call {
    long long begin, size;      // its positions in the output: [begin, begin + size)
    long long key;              // its key (a sequence's calls; else key_ids says)
};

// What a launch samples.  Two calling modes: one call over `total_all` positions keyed by key_ids[i % n_keys]  (offsets ==
// nullptr), or a SEQUENCE of calls c = 0..n_calls-1, call c drawing positions [offsets[c], offsets[c+1]) for the single key
// keys[c] -- each call completes its re-draw rounds before the next one draws, exactly like consecutive sample_by_user_ids
// calls on one numpy stream (the evaluation loader samples user by user, general_dataloader.py:141-146).
struct Calls {
    const int64_t* key_ids;
    long long n_keys, total_all;
    const int64_t* keys;
    const int64_t* offsets;
    long long n_calls;
    __device__ __forceinline__ long long count() const { return offsets ? n_calls : 1; }
    __device__ __forceinline__ long long end() const { return offsets ? offsets[n_calls] : total_all; }
    __device__ __forceinline__ Call at(long long c) const {      // (read once per call: three scalar loads in flight together)
        const long long o0 = offsets ? offsets[c] : 0;
        return {o0, offsets ? offsets[c + 1] - o0 : total_all, keys ? keys[c] : -1};
    }
};

struct UsedSets {      // CSR: the items of user u, ascending, are items[indptr[u] .. indptr[u + 1])
    const int64_t* indptr;
    const int32_t* items;
    long long n_users;
};

// One call: `draw(out, list, need)` draws a round of `need` values from the continuing stream (false: give the call up), the
// positions that hit their key's used-set form the next round, until none is left.  Draw::can_collide(v): may value v be in a
// used-set at all.
template <class Draw>
__device__ __forceinline__ bool sample_call(Draw& draw, const Calls& calls, const Call& c, const UsedSets& used,
                                            int64_t* __restrict__ out_all, int32_t* list_a, int32_t* list_b, BlockScan& sc,
                                            uint32_t* err, int& rounds) {
    int64_t* __restrict__ out = out_all + c.begin;
    const int32_t* list = nullptr;      // positions to (re)draw, ascending; nullptr = all of [0, total)
    int32_t* next = list_a;
    long long need = c.size;
    bool done = true;
    while (need > 0) {
        if (!draw(out, list, need)) {
            done = false;
            break;
        }
        ++rounds;
        if (!used.indptr) break;
        __threadfence_block();
        need = compact_hits(need, list, next, sc, [&](long long i) {
            const long long u = calls.keys ? c.key : calls.key_ids[i % calls.n_keys];
            if (u < 0 || u >= used.n_users) {
                if (err) atomicOr(err, FR_DEV_ERR_INDEX_RANGE);
                return false;
            }
            const long long v = out[i];
            return Draw::can_collide(v) && used_contains(used.items, used.indptr[u], used.indptr[u + 1], (int)v);
        });
        list = next;
        next = (next == list_a) ? list_b : list_a;
    }
    __syncthreads();   // the next call reuses the collision lists
    return done;
}

// a round of uniform values: np.random.randint(low, high, need)
struct UniformDraw {
    Stream& s;
    BlockScan& sc;
    long long low;
    uint32_t span, mask;
    __device__ static __forceinline__ bool can_collide(long long) { return true; }
    __device__ __forceinline__ bool operator()(int64_t* __restrict__ out, const int32_t* list, long long need) {
        draw_bounded(s, sc, low, span, mask, out, list, need);
        return true;
    }
};

// the calls of `calls` one after the other, uniform values (span > 0); returns the rounds drawn in all
__device__ __forceinline__ int uniform_calls(Stream& s, BlockScan& sc, long long low, uint32_t span, uint32_t mask, const Calls& calls,
                                             const UsedSets& used, int64_t* __restrict__ out_all, int32_t* list_a, int32_t* list_b,
                                             uint32_t* err) {
    UniformDraw draw{s, sc, low, span, mask};
    int rounds = 0;
    for (long long call = 0; call < calls.count(); ++call)
        sample_call(draw, calls, calls.at(call), used, out_all, list_a, list_b, sc, err, rounds);
    return rounds;
}

__global__ __launch_bounds__(SAMPLER_THREADS) void sample_negatives_kernel(
    uint32_t* __restrict__ state, long long low, uint32_t span, uint32_t mask, const int64_t* __restrict__ key_ids,
    long long n_keys, long long total_all, const int64_t* __restrict__ call_keys,
    const int64_t* __restrict__ call_offsets, long long n_calls, const int64_t* __restrict__ used_indptr,
    const int32_t* __restrict__ used_items, long long n_users, int64_t* __restrict__ out_all,
    int32_t* __restrict__ list_a, int32_t* __restrict__ list_b, int32_t* __restrict__ rounds_out, uint32_t* err) {
    __shared__ uint32_t mt[2][MT_N];
    __shared__ BlockScan sc;
    const int t = threadIdx.x;
    const Calls calls{key_ids, n_keys, total_all, call_keys, call_offsets, n_calls};
    Stream s{mt};
    s.load(state, t);
    __syncthreads();

    if (span == 0) {   // numpy: a one-value range consumes nothing
        const long long n_out = calls.end();
        for (long long e = t; e < n_out; e += SAMPLER_THREADS) out_all[e] = low;
        if (t == 0 && rounds_out) rounds_out[0] = 1;
        return;
    }

    const int rounds = uniform_calls(s, sc, low, span, mask, calls, UsedSets{used_indptr, used_items, n_users}, out_all, list_a,
                                     list_b, err);
    __syncthreads();
    s.store(state, t);
    if (t == 0 && rounds_out) rounds_out[0] = rounds;
}

// ---- A long SEQUENCE of single-key calls, resolved speculatively ------------------------------------------------------
// The evaluation loader draws user by user (general_dataloader.py:141-146): thousands of calls of 101-303 values per batch of
// users, each of which must finish its re-draw rounds before the next one draws.  Call by call that is ~11 us of barriers per
// call in sample_negatives_kernel -- 30 ms per evaluation batch, 200 times the scoring and ranking of the batch.  But the
// stream's ACCEPTED values (tempered word & mask <= span) are a function of the generator alone, a call consumes them in order
// -- its positions first, then one more per collision with the user's used-set, round by round -- and collisions are rare
// (|used-set| / n_items per draw).  So: (A) the accepted values of the whole sequence, plus slack, are generated once (the
// twist is the only sequential part: ~1.5 us per 624 words), each with its raw index in the stream and the generator block it
// came from kept; (B) every call is laid out as if NO call before it had collided, shifted by D = the extra values consumed so
// far; the first call with a collision is found in parallel, everything before it is final, that one call is resolved round
// by round exactly as the sequential kernel does, D grows by what it consumed beyond its size, and the search resumes behind
// it.  The generator state handed back is the block of the last consumed raw word and the position behind it: the same
// values, the same stream position as call-by-call consumption (tests/test_sampler_calls_hip.py holds both forms against numpy,
// path by path).
// If the slack does not suffice (a pathological collision rate), nothing has been published yet and the sequence runs call by
// call from the start.
static constexpr int CALLS_WINDOW = 1 << 16;      // positions examined per search for the next colliding call

// (A) The accepted values.  A1, one small workgroup that does nothing but twist the generator's blocks in LDS, every block kept
// (sample_calls_twist_kernel; the call-by-call kernel's 1024 threads spend four barriers per block AND temper, mask, scan).
// The block count is what the wanted number of accepted values needs at the mask's acceptance rate plus a margin; should
// chance leave fewer, (B) sees it and falls back.  A2, one wave per block over the chip: temper, mask, count the accepted
// words.  A3, the same waves again: each sums the counts of the blocks before its own and writes its accepted words, with
// their raw index in the stream, at their places.
__device__ __forceinline__ long long calls_want(long long total) { return total + (total / 32 > 1024 ? total / 32 : 1024); }

__global__ __launch_bounds__(256) void sample_calls_twist_kernel(const uint32_t* __restrict__ state, uint32_t span, uint32_t mask,
                                                                 const int64_t* __restrict__ call_offsets, long long n_calls,
                                                                 long long cap, uint32_t* __restrict__ snap, long long nblk_max,
                                                                 long long* __restrict__ hdr) {
    // Word n of the stream needs words n - 227, n - 623 and n - 624: a block of 624 is three dependent phases of <= 227 words.
    // Four waves, two copies of the block (old -> new, so that no phase overwrites what a neighbour still reads), one barrier
    // per phase: ~0.3 us per block (one wave walking the block 64 words at a time in place: 1.2 us).
    __shared__ uint32_t buf[2][MT_N];
    const int t = threadIdx.x;
    MtStream<256> s{buf};
    s.load(state, t);
    const int pos0 = s.pos;
    long long want = calls_want(call_offsets[n_calls]);
    if (want > cap) want = cap;
    // blocks beyond the incoming one: accepted words per block = 624 (span + 1) / (mask + 1) on average, 6 % and two blocks spare
    const double rate = ((double)span + 1.0) / ((double)mask + 1.0);
    long long need = want - (long long)((MT_N - pos0) * rate * 0.9);
    long long nblk = need > 0 ? (long long)((double)need / (MT_N * rate * 0.94)) + 2 : 0;
    if (nblk > nblk_max - 1) nblk = nblk_max - 1;
    __syncthreads();
    // (the phases hand LDS words to each other: the barrier waits for this wave's LDS traffic only, not for the block copies
    // on their way to global memory, which __syncthreads' fence would drain three times per block)
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    for (int k = t; k < MT_N; k += 256) snap[k] = s.block()[k];      // the incoming block
    for (long long blk = 1; blk <= nblk; ++blk) {
        const uint32_t* __restrict__ o = s.block();
        uint32_t* __restrict__ n = s.other();
        if (t < MT_H) n[t] = mt_next_word(o, n, t);
        lds_barrier();
        if (t < MT_H) n[MT_H + t] = mt_next_word(o, n, MT_H + t);
        lds_barrier();
        if (2 * MT_H + t < MT_N) n[2 * MT_H + t] = mt_next_word(o, n, 2 * MT_H + t);
        lds_barrier();
        s.flip();
        for (int k = t; k < MT_N; k += 256) snap[blk * MT_N + k] = s.block()[k];
    }
    if (t == 0) {
        hdr[1] = nblk + 1;      // blocks kept, the incoming one included
        hdr[2] = pos0;
        hdr[3] = want;
    }
}

// PASS 0: cnt[blk] = accepted words of block blk; PASS 1: the words themselves, behind those of the blocks before
template <int PASS>
__global__ __launch_bounds__(64) void sample_calls_temper_kernel(uint32_t span, uint32_t mask, const uint32_t* __restrict__ snap,
                                                                 long long* __restrict__ hdr, uint32_t* __restrict__ cnt,
                                                                 uint32_t* __restrict__ acc_val, uint32_t* __restrict__ acc_raw) {
    const long long blk = blockIdx.x, nblk = hdr[1];
    if (blk >= nblk) return;
    const int l = threadIdx.x, pos = blk == 0 ? (int)hdr[2] : 0;
    const long long want = hdr[3];
    long long before = 0;
    if (PASS == 1) {
        for (long long b0 = 0; b0 < blk; b0 += 64) before += b0 + l < blk ? cnt[b0 + l] : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) before += __shfl_xor((int)before, o, 64);      // (below 2^31: the buffers hold < 2^30 values)
    }
    long long produced = before;
    for (int k0 = pos & ~63; k0 < MT_N; k0 += 64) {
        const int k = k0 + l;
        uint32_t v = 0;
        bool acc = false;
        if (k >= pos && k < MT_N) {
            v = mt_temper(snap[blk * MT_N + k]) & mask;
            acc = v <= span;
        }
        const unsigned long long bal = __ballot(acc);
        if (PASS == 1) {
            const long long e = produced + __popcll(bal & ((1ull << l) - 1ull));
            if (acc && e < want) {
                acc_val[e] = v;
                acc_raw[e] = (uint32_t)(blk * MT_N + k);
            }
        }
        produced += __popcll(bal);
    }
    if (PASS == 0 && l == 0) cnt[blk] = (uint32_t)(produced - before);
    if (PASS == 1 && l == 0 && blk == nblk - 1) hdr[0] = produced < want ? produced : want;      // accepted values available
}

// (P) every position of the sequence, in parallel over the chip: its call, and for each shift d < CALLS_SHIFTS whether the
// accepted value it would take under that shift (acc_val[p + d]) lies in its user's used-set -- one bit per shift.  The
// sequential part (B) then finds "the first position that collides under the current shift" by reading one word per position.
// hmask and pos_call hold lo_t positions (the capacity the workspace was laid out for): a longer sequence is left to (B)'s
// call-by-call fallback.
static constexpr int CALLS_SHIFTS = 32;
__global__ __launch_bounds__(256) void sample_calls_hits_kernel(long long low, const int64_t* __restrict__ call_keys,
                                                                const int64_t* __restrict__ call_offsets, long long n_calls,
                                                                long long lo_t,
                                                                const int64_t* __restrict__ used_indptr,
                                                                const int32_t* __restrict__ used_items, long long n_users,
                                                                const uint32_t* __restrict__ acc_val,
                                                                const long long* __restrict__ n_acc_in, uint32_t* __restrict__ hmask,
                                                                int32_t* __restrict__ pos_call, uint32_t* err) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = call_offsets[n_calls];
    if (p >= total || p >= lo_t) return;
    long long a = 0, b = n_calls - 1;      // the call of position p: the largest c with call_offsets[c] <= p
    while (a < b) {
        const long long mid = (a + b + 1) >> 1;
        if (call_offsets[mid] <= p) a = mid;
        else b = mid - 1;
    }
    pos_call[p] = (int32_t)a;
    const long long u = call_keys[a];
    uint32_t bits = 0;
    if (u < 0 || u >= n_users) {
        if (err) atomicOr(err, FR_DEV_ERR_INDEX_RANGE);
    } else {
        const long long ulo = used_indptr[u], uhi = used_indptr[u + 1];
        const long long n_acc = n_acc_in[0];
        if (uhi > ulo) {
#pragma unroll 4
            for (int d = 0; d < CALLS_SHIFTS; ++d)
                if (p + d < n_acc && used_contains(used_items, ulo, uhi, (int)(low + (long long)acc_val[p + d]))) bits |= 1u << d;
        }
    }
    hmask[p] = bits;
}

// (B) ONE workgroup: the calls in order, everything before the next colliding position final
__global__ __launch_bounds__(SAMPLER_THREADS) void sample_calls_fast_kernel(
    uint32_t* __restrict__ state, long long low, uint32_t span, uint32_t mask, const int64_t* __restrict__ call_keys,
    const int64_t* __restrict__ call_offsets, long long n_calls, long long lo_t, const int64_t* __restrict__ used_indptr,
    const int32_t* __restrict__ used_items, long long n_users, int64_t* __restrict__ out, const uint32_t* __restrict__ acc_val,
    const uint32_t* __restrict__ acc_raw, const uint32_t* __restrict__ snap, const long long* __restrict__ n_acc_in,
    const uint32_t* __restrict__ hmask, const int32_t* __restrict__ pos_call, int32_t* list_a, int32_t* list_b, uint32_t* err) {
    __shared__ uint32_t mt[2][MT_N];
    __shared__ BlockScan sc;
    __shared__ long long s_first;
    const int t = threadIdx.x;
    const long long total = call_offsets[n_calls];
    const long long n_acc = n_acc_in[0];
    long long D = 0, p0 = 0;     // positions before p0 are final; D = accepted values consumed beyond the positions so far
    bool over = total > lo_t || total + D > n_acc;      // (more positions than the layout holds: call by call)
    while (p0 < total && !over) {
        const long long pe = p0 + CALLS_WINDOW < total ? p0 + CALLS_WINDOW : total;
        if (t == 0) s_first = pe;
        __syncthreads();
        long long mine = pe;
        for (long long p = p0 + t; p < pe; p += SAMPLER_THREADS)
            if ((hmask[p] >> D) & 1u) {
                mine = p;
                break;
            }
        if (mine < pe) atomicMin((unsigned long long*)&s_first, (unsigned long long)mine);
        __syncthreads();
        const long long pf0 = s_first;                       // the first colliding position of the window (pe: none)
        const long long cf = pf0 < pe ? pos_call[pf0] : -1;
        const long long pf = cf >= 0 ? call_offsets[cf] : pe;      // the positions before the colliding call are final
        if (pf + D > n_acc) {
            over = true;
            break;
        }
        for (long long p = p0 + t; p < pf; p += SAMPLER_THREADS) out[p] = low + (long long)acc_val[p + D];
        __syncthreads();
        if (cf < 0) {
            p0 = pe;
            continue;
        }
        // the colliding call, round by round: its positions take the next accepted values in position order, the positions that
        // hit the used-set take the values behind those, and so on
        const long long n = call_offsets[cf + 1] - pf, base = pf + D;
        const long long u = call_keys[cf];
        const long long ulo = used_indptr[u], uhi = used_indptr[u + 1];
        const int32_t* list = nullptr;
        int32_t* next = list_a;
        long long need = n, consumed = 0;
        while (need > 0) {
            if (base + consumed + need > n_acc) {
                over = true;
                break;
            }
            for (long long e = t; e < need; e += SAMPLER_THREADS)
                out[pf + (list ? (long long)list[e] : e)] = low + (long long)acc_val[base + consumed + e];
            __threadfence_block();
            __syncthreads();
            consumed += need;
            need = compact_hits(need, list, next, sc,
                                [&](long long i) { return used_contains(used_items, ulo, uhi, (int)out[pf + i]); });
            list = next;
            next = (next == list_a) ? list_b : list_a;
        }
        if (over) break;
        D += consumed - n;
        p0 = pf + n;
        if (D >= CALLS_SHIFTS) over = true;      // (the hit bits cover CALLS_SHIFTS shifts)
    }
    __syncthreads();
    if (over) {
        // too many collisions for the slack / the shifts prepared: call by call from the incoming state, as
        // sample_negatives_kernel runs a sequence (nothing of the stream was published; the outputs written so far are
        // overwritten)
        Stream s{mt};
        s.load(state, t);
        __syncthreads();
        uniform_calls(s, sc, low, span, mask, Calls{nullptr, 1, 0, call_keys, call_offsets, n_calls},
                      UsedSets{used_indptr, used_items, n_users}, out, list_a, list_b, err);
        __syncthreads();
        s.store(state, t);
        return;
    }
    // the generator after the last consumed word
    const long long E = total + D;
    if (E > 0) {
        const uint32_t R = acc_raw[E - 1];
        const long long bf = R / MT_N;
        if (t < MT_N) state[t] = snap[bf * MT_N + t];
        if (t == 0) state[MT_N] = (uint32_t)(R % MT_N) + 1u;
    }
}

// ---- Popularity-biased negatives -------------------------------------------------------------------------------------
// Replaces: recbole/sampler/sampler.py Sampler._pop_sampling (the alias method over the items of every phase's interactions)
// inside the same rejection loop of sample_by_key_ids.  A round over the m positions still open draws
//   idx  = np.random.randint(0, n, m)   -- masked rejection on single words, span n - 1 (no words at all when n == 1)
//   coin = np.random.random(m)          -- 2m consecutive raw words, coin = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 in fp64
//   value = keys[idx] if prob[idx] > coin else alias[idx]   (alias copied verbatim, -1 included)
// and the positions whose value is in the key's used-set, in ascending order, form the next round.  The structure is
// sample_negatives_kernel's: one workgroup runs every round of every call (sample_call), the state stays in LDS between them.
// A call that is still open after POP_MAX_ROUNDS rounds stops the launch with FR_DEV_ERR_SAMPLE_ROUNDS instead of spinning:
// with 32768 positions open that takes a used-set carrying more than 99.998 % of the popularity mass, and a used-set that
// covers every key (the reference loops forever) is refused on the host before any launch (fairrec/sampler/sampler.py).
static constexpr int POP_MAX_ROUNDS = 1 << 20;

// a round of popularity-biased values: slots, then coins
struct PopDraw {
    Stream& s;
    BlockScan& sc;
    uint32_t& carry;      // (LDS) first word of a coin whose second word lies behind the next twist
    const int64_t* tab_keys;
    const double* tab_prob;
    const int64_t* tab_alias;
    uint32_t span, mask;
    uint32_t* err;
    int call_rounds;      // rounds of the current call
    __device__ static __forceinline__ bool can_collide(long long v) { return v >= 0; }      // (alias -1: never in a used-set)
    __device__ __forceinline__ bool operator()(int64_t* __restrict__ out, const int32_t* list, long long need) {
        const int t = threadIdx.x;
        if (call_rounds == POP_MAX_ROUNDS) {
            if (t == 0 && err) atomicOr(err, FR_DEV_ERR_SAMPLE_ROUNDS);
            return false;
        }
        ++call_rounds;
        // ---- slots: np.random.randint(0, n, need), the uniform kernel's draw with low = 0 ----
        if (span == 0) {
            for (long long e = t; e < need; e += SAMPLER_THREADS) out[list ? (long long)list[e] : e] = 0;
        } else {
            draw_bounded(s, sc, 0, span, mask, out, list, need);
        }
        __syncthreads();
        __threadfence_block();
        // ---- coins: np.random.random(need) = the next 2 * need raw words; word r of the phase is word 2e + (r & 1) of
        // position e.  A pair split by a twist (the phase can start at either parity) passes its first word on in `carry`.
        const long long cw = 2 * need;
        long long cdone = 0;
        while (cdone < cw) {
            s.refill(t);
            const uint32_t* w = s.block();
            const int pos = s.pos;
            const int take = (int)(cw - cdone < (long long)(MT_N - pos) ? cw - cdone : (long long)(MT_N - pos));
            if (t >= pos && t < pos + take) {
                const long long r = cdone + (t - pos);
                uint32_t w0 = 0, w1 = 0;
                bool pair = false;
                if ((r & 1) == 0) {
                    if (t + 1 < pos + take) {
                        w0 = mt_temper(w[t]);
                        w1 = mt_temper(w[t + 1]);
                        pair = true;
                    } else {
                        carry = mt_temper(w[t]);      // (t == MT_N - 1: the second word is the next block's first)
                    }
                } else if (t == pos) {
                    w0 = carry;
                    w1 = mt_temper(w[t]);
                    pair = true;
                }
                if (pair) {
                    const long long e = r >> 1;
                    const long long i = list ? (long long)list[e] : e;
                    const long long slot = out[i];
                    const double coin = ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
                    out[i] = tab_prob[slot] > coin ? tab_keys[slot] : tab_alias[slot];
                }
            }
            __syncthreads();
            s.pos += take;
            cdone += take;
        }
        return true;
    }
};

__global__ __launch_bounds__(SAMPLER_THREADS) void sample_negatives_pop_kernel(
    uint32_t* __restrict__ state, const int64_t* __restrict__ tab_keys, const double* __restrict__ tab_prob,
    const int64_t* __restrict__ tab_alias, uint32_t span, uint32_t mask, const int64_t* __restrict__ key_ids,
    long long n_keys, long long total_all, const int64_t* __restrict__ call_keys, const int64_t* __restrict__ call_offsets,
    long long n_calls, long long max_call, const int64_t* __restrict__ used_indptr, const int32_t* __restrict__ used_items,
    long long n_users, int64_t* __restrict__ out_all, int32_t* __restrict__ list_a, int32_t* __restrict__ list_b,
    int32_t* __restrict__ rounds_out, uint32_t* err) {
    __shared__ uint32_t mt[2][MT_N];
    __shared__ BlockScan sc;
    __shared__ uint32_t s_carry;
    const int t = threadIdx.x;
    const Calls calls{key_ids, n_keys, total_all, call_keys, call_offsets, n_calls};
    const UsedSets used{used_indptr, used_items, n_users};
    Stream s{mt};
    s.load(state, t);
    __syncthreads();

    PopDraw draw{s, sc, s_carry, tab_keys, tab_prob, tab_alias, span, mask, err, 0};
    int rounds = 0;
    for (long long call = 0; call < calls.count(); ++call) {
        const Call c = calls.at(call);
        if (c.size > max_call) {      // (the collision lists hold max_call positions)
            if (t == 0 && err) atomicOr(err, FR_DEV_ERR_INDEX_RANGE);
            continue;
        }
        draw.call_rounds = 0;
        if (!sample_call(draw, calls, c, used, out_all, list_a, list_b, sc, err, rounds)) break;      // (stuck)
    }
    __syncthreads();
    s.store(state, t);
    if (t == 0 && rounds_out) rounds_out[0] = rounds;
}

// mt19937_seed(state, seed): Knuth's LCG over the 624 words, pos = 624 (np.random.seed(int))
__global__ void mt19937_seed_kernel(uint32_t* __restrict__ state, uint32_t seed) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t s = seed;
    for (int i = 0; i < MT_N; ++i) {
        state[i] = s;
        s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i + 1u;
    }
    state[MT_N] = MT_N;
}

}  // namespace fr

using namespace fr;

extern "C" int fr_mt19937_seed(uint32_t* state, uint32_t seed, void* stream_) {
    FR_CHECK_ARG(state, "fr_mt19937_seed: null state");
    hipLaunchKernelGGL(mt19937_seed_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, state, seed);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" size_t fr_sample_negatives_workspace_bytes(int64_t total) {
    return total < 1 ? 0 : 2 * align_up((size_t)total * sizeof(int32_t), 256);
}

// the two collision lists of calls of at most max_call positions, in fr_sample_negatives_workspace_bytes(max_call) bytes
struct CollisionLists {
    int32_t *a = nullptr, *b = nullptr;
};
static CollisionLists split_lists(void* ws, int64_t max_call) {
    return {(int32_t*)ws, (int32_t*)((char*)ws + align_up((size_t)max_call * sizeof(int32_t), 256))};
}

static int sample_launch(uint32_t* state, int64_t low, int64_t high, const int64_t* key_ids, int64_t n_keys, int64_t total,
                         const int64_t* call_keys, const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                         const int64_t* used_indptr, const int32_t* used_items, int64_t n_users, int64_t* out,
                         int32_t* rounds_out, void* ws, size_t ws_bytes, uint32_t* err_flag, hipStream_t stream) {
    FR_CHECK_ARG(!used_indptr || (ws && ws_bytes >= fr_sample_negatives_workspace_bytes(max_call)),
                 "fr_sample_negatives: workspace too small");
    const CollisionLists lists = used_indptr ? split_lists(ws, max_call) : CollisionLists{};
    const uint32_t span = (uint32_t)(high - 1 - low);
    ProfScope prof(K_SAMPLE_NEG, stream);
    FR_LAUNCH(prof, sample_negatives_kernel, dim3(1), dim3(SAMPLER_THREADS), 0, stream, state, (long long)low, span,
              bounded_mask(span), key_ids, (long long)n_keys, (long long)total, call_keys, call_offsets, (long long)n_calls,
              used_indptr, used_items, (long long)n_users, out, lists.a, lists.b, rounds_out, err_flag);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_sample_negatives(uint32_t* state, int64_t low, int64_t high, const int64_t* key_ids, int64_t n_keys,
                                   int32_t num, const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                                   int64_t* out, int32_t* rounds_out, void* ws, size_t ws_bytes, uint32_t* err_flag,
                                   void* stream_) {
    FR_CHECK_ARG(state && out && n_keys >= 1 && num >= 1 && n_keys * (int64_t)num <= (1ll << 30),
                 "fr_sample_negatives: bad size");
    FR_CHECK_ARG(high > low && high - 1 - low < 0xffffffffll, "fr_sample_negatives: range [%lld, %lld) not below 2^32",
                 (long long)low, (long long)high);
    FR_CHECK_ARG(!used_indptr || (used_items && key_ids && n_users >= 1 && ws), "fr_sample_negatives: used-set arguments");
    const int64_t total = n_keys * (int64_t)num;
    return sample_launch(state, low, high, key_ids, n_keys, total, nullptr, nullptr, 1, total, used_indptr, used_items,
                         n_users, out, rounds_out, ws, ws_bytes, err_flag, (hipStream_t)stream_);
}

// ---- a sequence of single-key calls on one stream: call c fills out[call_offsets[c] .. call_offsets[c+1]) for key
// call_keys[c]; `max_call` >= the longest call sizes the collision lists -----------------------------------------------
// Workspace of the speculative form of a sequence of `total` values in all: byte offsets of its parts, in this order
// (tests/sampler_ref.py restates the sizes).
struct CallsLayout {
    size_t cap, nblk;      // accepted values kept; generator blocks kept
    size_t acc_val;        // accepted values
    size_t acc_raw;        // ... their raw indices
    size_t blocks;         // the generator's blocks
    size_t lists;          // collision lists a, b of the call being resolved
    size_t hdr;            // (accepted values available, blocks kept, incoming position, values wanted)
    size_t hit_bits;       // per position: for which shifts it collides
    size_t pos_call;       // ... and its call
    size_t blk_cnt;        // accepted words per block
    size_t bytes;
};
static CallsLayout calls_fast_layout(int64_t total, int64_t max_call) {
    CallsLayout L;
    L.cap = (size_t)total + std::max<size_t>(1024, (size_t)total / 32);
    L.nblk = 2 * L.cap / MT_N + 4;      // the mask keeps more than every second word
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += align_up(b, 256); return at; };
    L.acc_val = take(L.cap * 4);
    L.acc_raw = take(L.cap * 4);
    L.blocks = take(L.nblk * MT_N * 4);
    L.lists = take(fr_sample_negatives_workspace_bytes(max_call));
    L.hdr = take(32);
    L.hit_bits = take((size_t)total * 4);
    L.pos_call = take((size_t)total * 4);
    L.blk_cnt = take(L.nblk * 4);
    L.bytes = o;
    return L;
}
extern "C" size_t fr_sample_negatives_calls_workspace_bytes(int64_t total, int64_t max_call) {
    return total < 1 || max_call < 1 ? 0 : calls_fast_layout(total, max_call).bytes;
}

// the speculative form in a workspace laid out for lo_t positions: twist, count, place, hit bits, resolve
static int calls_fast_launch(const CallsLayout& L, int64_t lo_t, uint32_t* state, int64_t low, uint32_t span,
                             const int64_t* call_keys, const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                             const int64_t* used_indptr, const int32_t* used_items, int64_t n_users, int64_t* out, void* ws,
                             uint32_t* err_flag, hipStream_t stream) {
    char* w = (char*)ws;
    uint32_t *acc_val = (uint32_t*)(w + L.acc_val), *acc_raw = (uint32_t*)(w + L.acc_raw), *blocks = (uint32_t*)(w + L.blocks);
    uint32_t *hit_bits = (uint32_t*)(w + L.hit_bits), *blk_cnt = (uint32_t*)(w + L.blk_cnt);
    long long* hdr = (long long*)(w + L.hdr);
    int32_t* pos_call = (int32_t*)(w + L.pos_call);
    const CollisionLists lists = split_lists(w + L.lists, max_call);
    const uint32_t mask = bounded_mask(span);
    ProfScope prof(K_SAMPLE_NEG, stream);
    FR_LAUNCH(prof, sample_calls_twist_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t*)state, span, mask, call_offsets,
              (long long)n_calls, (long long)L.cap, blocks, (long long)L.nblk, hdr);
    FR_LAUNCH(prof, sample_calls_temper_kernel<0>, dim3((unsigned)L.nblk), dim3(64), 0, stream, span, mask,
              (const uint32_t*)blocks, hdr, blk_cnt, acc_val, acc_raw);
    FR_LAUNCH(prof, sample_calls_temper_kernel<1>, dim3((unsigned)L.nblk), dim3(64), 0, stream, span, mask,
              (const uint32_t*)blocks, hdr, blk_cnt, acc_val, acc_raw);
    FR_LAUNCH(prof, sample_calls_hits_kernel, dim3((unsigned)((lo_t + 255) / 256)), dim3(256), 0, stream, (long long)low,
              call_keys, call_offsets, (long long)n_calls, (long long)lo_t, used_indptr, used_items, (long long)n_users,
              (const uint32_t*)acc_val, (const long long*)hdr, hit_bits, pos_call, err_flag);
    FR_LAUNCH(prof, sample_calls_fast_kernel, dim3(1), dim3(SAMPLER_THREADS), 0, stream, state, (long long)low, span, mask,
              call_keys, call_offsets, (long long)n_calls, (long long)lo_t, used_indptr, used_items, (long long)n_users, out,
              (const uint32_t*)acc_val, (const uint32_t*)acc_raw, (const uint32_t*)blocks, (const long long*)hdr,
              (const uint32_t*)hit_bits, (const int32_t*)pos_call, lists.a, lists.b, err_flag);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_sample_negatives_calls(uint32_t* state, int64_t low, int64_t high, const int64_t* call_keys,
                                         const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                                         const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                                         int64_t* out, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream_) {
    FR_CHECK_ARG(state && out && call_keys && call_offsets && n_calls >= 1 && max_call >= 1 && max_call <= (1ll << 30),
                 "fr_sample_negatives_calls: bad argument");
    FR_CHECK_ARG(high > low && high - 1 - low < 0xffffffffll, "fr_sample_negatives_calls: range not below 2^32");
    FR_CHECK_ARG(used_indptr && used_items && n_users >= 1 && ws, "fr_sample_negatives_calls: used-set arguments");
    // With a workspace of fr_sample_negatives_calls_workspace_bytes(total, max_call) a sequence of many calls is resolved
    // speculatively (sample_calls_fast_kernel); `total` is not known to the host without a synchronisation, so the caller says
    // how much room there is and the size is read back from it: the layout for lo_t = the largest total the workspace holds
    // is what the kernels use (they stop generating at its capacity, mark hits for its first lo_t positions only, and fall
    // back call by call if the total exceeds lo_t or the accepted values fall short).
    if (n_calls >= 16 && high - 1 - low > 0) {
        // the largest `total` whose layout fits the workspace (bisection on the monotone size function)
        int64_t lo_t = 0, hi_t = (int64_t)1 << 30;
        while (lo_t < hi_t) {
            const int64_t mid = (lo_t + hi_t + 1) >> 1;
            if (fr_sample_negatives_calls_workspace_bytes(mid, max_call) <= ws_bytes) lo_t = mid;
            else hi_t = mid - 1;
        }
        if (lo_t >= n_calls)      // (else a workspace sized for the call-by-call form only: no room)
            return calls_fast_launch(calls_fast_layout(lo_t, max_call), lo_t, state, low, (uint32_t)(high - 1 - low), call_keys,
                                     call_offsets, n_calls, max_call, used_indptr, used_items, n_users, out, ws, err_flag,
                                     (hipStream_t)stream_);
    }
    return sample_launch(state, low, high, nullptr, 1, 0, call_keys, call_offsets, n_calls, max_call, used_indptr, used_items,
                         n_users, out, nullptr, ws, ws_bytes, err_flag, (hipStream_t)stream_);
}

// ---- popularity-biased negatives: argument checks, then one launch of sample_negatives_pop_kernel ------------------------
static int pop_launch(uint32_t* state, const fr_alias_table* table, const int64_t* key_ids, int64_t n_keys, int64_t total,
                      const int64_t* call_keys, const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                      const int64_t* used_indptr, const int32_t* used_items, int64_t n_users, int64_t* out,
                      int32_t* rounds_out, void* ws, uint32_t* err_flag, hipStream_t stream) {
    const CollisionLists lists = used_indptr ? split_lists(ws, max_call) : CollisionLists{};
    const uint32_t span = (uint32_t)(table->n - 1);
    ProfScope prof(K_SAMPLE_NEG, stream);
    FR_LAUNCH(prof, sample_negatives_pop_kernel, dim3(1), dim3(SAMPLER_THREADS), 0, stream, state, table->keys, table->prob,
              table->alias, span, bounded_mask(span), key_ids, (long long)n_keys, (long long)total, call_keys, call_offsets,
              (long long)n_calls, (long long)max_call, used_indptr, used_items, (long long)n_users, out, lists.a, lists.b,
              rounds_out, err_flag);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

#define FR_CHECK_ALIAS_TABLE(table, who)                                                                                   \
    FR_CHECK_ARG(table && table->keys && table->prob && table->alias, who ": null table pointer");                          \
    FR_CHECK_ARG(table->n >= 1 && table->n - 1 < 0xffffffffll, who ": table of %lld keys (1 .. 2^32 - 1)", (long long)table->n)

extern "C" int fr_sample_negatives_pop(uint32_t* state, const fr_alias_table* table, const int64_t* key_ids, int64_t n_keys,
                                       int32_t num, const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                                       int64_t* out, int32_t* rounds_out, void* ws, size_t ws_bytes, uint32_t* err_flag,
                                       void* stream_) {
    FR_CHECK_ALIAS_TABLE(table, "fr_sample_negatives_pop");
    FR_CHECK_ARG(state && out && n_keys >= 1 && num >= 1 && n_keys <= (1ll << 30) && n_keys * (int64_t)num <= (1ll << 30),
                 "fr_sample_negatives_pop: bad size");
    FR_CHECK_ARG(!used_indptr || (used_items && key_ids && n_users >= 1 && ws), "fr_sample_negatives_pop: used-set arguments");
    const int64_t total = n_keys * (int64_t)num;
    FR_CHECK_ARG(!used_indptr || ws_bytes >= fr_sample_negatives_workspace_bytes(total), "fr_sample_negatives_pop: workspace too small");
    return pop_launch(state, table, key_ids, n_keys, total, nullptr, nullptr, 1, total, used_indptr, used_items, n_users, out,
                      rounds_out, ws, err_flag, (hipStream_t)stream_);
}

extern "C" int fr_sample_negatives_pop_calls(uint32_t* state, const fr_alias_table* table, const int64_t* call_keys,
                                             const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                                             const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                                             int64_t* out, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream_) {
    FR_CHECK_ALIAS_TABLE(table, "fr_sample_negatives_pop_calls");
    FR_CHECK_ARG(state && out && call_keys && call_offsets && n_calls >= 1 && max_call >= 1 && max_call <= (1ll << 30),
                 "fr_sample_negatives_pop_calls: bad size");
    FR_CHECK_ARG(used_indptr && used_items && n_users >= 1 && ws, "fr_sample_negatives_pop_calls: used-set arguments");
    FR_CHECK_ARG(ws_bytes >= fr_sample_negatives_workspace_bytes(max_call), "fr_sample_negatives_pop_calls: workspace too small");
    return pop_launch(state, table, nullptr, 1, 0, call_keys, call_offsets, n_calls, max_call, used_indptr, used_items, n_users,
                      out, nullptr, ws, err_flag, (hipStream_t)stream_);
}
