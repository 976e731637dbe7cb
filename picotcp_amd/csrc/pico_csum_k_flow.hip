// pico_csum_k_flow.hip -- flow grouping: a verified burst becomes the group-contiguous, arrival-ordered
// descriptors and the groups[] that the reassembly and coalescing batches take (pico_csum_k_frag.hip,
// pico_csum_k_tcprx.hip) -- and its launcher.  The batch form of the per-frame lookups of the reference:
// pico_socket_tcp_deliver (modules/pico_socket_tcp.c:125-226: remote port, remote address, local
// address) and the fragment trees' key (modules/pico_fragments.c:104-122, :160-178: id, source,
// destination).  Helpers and the IPv6 extension-header walk: pico_csum_dev.h.  The contract:
// include/pico_csum.h, pico_flow_group_batch_dev.
//
// One index space of N = n_known + n entries: entry e < n_known is the host's table key e, entry
// n_known + f is frame f.  A group's LEADER is its smallest entry: the table key, or the first arrival.
//   1. flow_parse    one lane per entry: the key (10 words), its hash and a valid flag into scratch;
//   2. flow_elect    one lane per valid entry: an open-addressed table of cap >= 2 N slots (one entry
//                    index each).  An empty slot is claimed with atomicCAS; an occupied one is compared
//                    by key with its occupant (whose key an EARLIER launch wrote) and, when equal, takes
//                    the smaller index with atomicMin.  Every occupant a slot ever has carries one key;
//   3. flow_resolve  one lane per frame: the same probe reads the slot's final occupant, the leader.
//                    The sort key of a frame is its leader, all ones when it is not selected;
//   4. a stable LSD radix sort of (leader, frame index), 8 bits a pass over the ceil(log2(N + 1)) key
//                    bits: radix_hist (per-tile digit counts), scan_excl (one workgroup, in place) and
//                    radix_scatter (rank inside the tile: per-digit ballots within a wave, an LDS
//                    prefix across the waves).  Sorted by leader, table groups come first in table
//                    order, then the other groups by first arrival, members by arrival, and the
//                    frames not selected last in ascending index;
//   5. flow_heads / scan_excl / flow_emit / flow_counts: run heads that are their own leader number the
//                    groups behind the table's; heads write a group's first slot, tails its end.
// Every loop is bounded by a value known on entry (probing: cap steps; a frame whose probe runs out
// is left unselected), no lane waits for another lane's store: the phases are ordered by launch.
#include "pico_csum_dev.h"

namespace {

constexpr uint32_t FLOW_TILE = 1024u;           // threads of a workgroup = elements of a radix / scan tile
constexpr uint32_t FLOW_WAVES = FLOW_TILE / 64u;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;         // a free table slot; the sort key of a frame not selected
constexpr uint32_t M_TCP = 1u, M_FRAG4 = 2u, M_FRAG6 = 3u, MF_ETH = 0x10u;   // include/pico_csum.h

struct FlowArgs {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* desc;
    uint32_t n;
    const uint8_t* verdict_in;
    uint32_t mode, eth;
    const uint8_t* known;               // struct pico_csum_flow_key[n_known], 40 bytes each
    uint32_t n_known, seed;
    pico_csum_desc_dev* o_desc;
    uint32_t* o_index;
    uint32_t* o_groups;
    uint32_t* o_counts;
    // scratch
    uint4* keys;                        // N entries of 12 words: 10 key words, the hash, the valid flag
    uint32_t* table;                    // cap slots
    uint32_t cap;                       // a power of two >= 2 N
    uint32_t* ka; uint32_t* va; uint32_t* kb; uint32_t* vb;   // the sort's two (key, value) buffers, n each
    uint32_t* hist;                     // 256 * ntiles digit counts; the emit's ntiles head counts
    uint32_t ntiles;
};

// Frame d's network header: false when the region (or, with F_ETH, its 14-byte Ethernet header) does not
// lie inside the batch.
__device__ __forceinline__ bool net_region(const FlowArgs& p, const pico_csum_desc_dev& d, uint64_t& off, uint32_t& avail) {
    off = 0;
    avail = 0;
    if (d.off > p.base_len || d.len > p.base_len - d.off) return false;
    const uint32_t skip = p.eth ? 14u : 0u;
    if (d.len < skip) return false;
    off = d.off + skip;
    avail = d.len - skip;
    return true;
}

__device__ __forceinline__ uint32_t flow_hash(const uint32_t (&k)[10], uint32_t seed) {
    uint32_t h = seed ^ 0x9E3779B9u;
#pragma unroll
    for (int m = 0; m < 10; ++m) {
        h ^= k[m];
        h *= 0x85EBCA6Bu;
        h = (h << 13) | (h >> 19);
    }
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// The key of frame f under the mode's parse rules (include/pico_csum.h): words 0-3 src, 4-7 dst, 8 =
// sport | dport << 16 (FRAG4: the id; FRAG6: the 32-bit id), 9 = family.  False: not selected.
__device__ __forceinline__ bool frame_key(const FlowArgs& p, uint32_t f, uint32_t (&k)[10]) {
#pragma unroll
    for (int m = 0; m < 10; ++m) k[m] = 0u;
    const pico_csum_desc_dev d = p.desc[f];
    uint64_t off;
    uint32_t avail;
    if (!net_region(p, d, off, avail)) return false;
    if (p.verdict_in) {
        const uint32_t want = p.mode == M_TCP ? V_ACCEPT : V_FRAG;
        if (((uint32_t)p.verdict_in[f] & ~V_IPV6) != want) return false;
    }
    if (avail < 20u) return false;
    const uint8_t* h = p.base + off;
    const uint32_t w0 = ld32(h);
    const uint32_t ver = (w0 & 0xFFu) >> 4;
    if (ver == 4u) {
        if (p.mode == M_FRAG6) return false;
        const uint32_t ihl = w0 & 0x0Fu;
        if (ihl < 5u) return false;
        const uint32_t w1 = ld32(h + 4), w2 = ld32(h + 8);
        const bool fragment = (((w1 >> 16) & 0xFFu) & 0x3Fu) != 0u || (w1 >> 24) != 0u;      // MF or an offset
        k[0] = ld32(h + 12);
        k[4] = ld32(h + 16);
        k[9] = 4u;
        if (p.mode == M_TCP) {
            if (((w2 >> 8) & 0xFFu) != 6u || fragment || 4u * ihl + 4u > avail) return false;
            k[8] = ld32(h + 4u * ihl);
        } else {
            if (!fragment) return false;
            k[8] = w1 & 0xFFFFu;                // the id as stored
        }
        return true;
    }
    if (ver == 6u) {
        if (p.mode == M_FRAG4 || avail < 40u) return false;
        if (p.mode == M_TCP) {
            if (avail < 44u || ((ld32(h + 4) >> 16) & 0xFFu) != 6u) return false;
            k[8] = ld32(h + 40);
        } else {
            const uint64_t w = ipv6_walk_packed(h, avail);
            if ((int)(w & 0xFFu) - 1 != WALK_FRAG) return false;
            const uint32_t fo = (uint32_t)(w >> 48);
            if (fo + 8u > avail) return false;
            k[8] = ld32(h + fo + 4u);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            k[m] = ld32(h + 8 + 4 * m);
            k[4 + m] = ld32(h + 24 + 4 * m);
        }
        k[9] = 6u;
        return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void flow_parse(FlowArgs p) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x, N = p.n + p.n_known;
    if (e >= N) return;
    uint32_t k[10];
    bool valid;
    if (e < p.n_known) {                // a table key as the host wrote it (reserved bytes not compared)
        const uint8_t* t = p.known + 40ull * e;
#pragma unroll
        for (int m = 0; m < 10; ++m) k[m] = ld32(t + 4 * m);
        k[9] &= 0xFFu;
        valid = true;
    } else {
        valid = frame_key(p, e - p.n_known, k);
    }
    uint4* K = p.keys + 3ull * e;
    K[0] = make_uint4(k[0], k[1], k[2], k[3]);
    K[1] = make_uint4(k[4], k[5], k[6], k[7]);
    K[2] = make_uint4(k[8], k[9], flow_hash(k, p.seed), valid ? 1u : 0u);
}

struct Key3 {
    uint4 a, b, c;
};
__device__ __forceinline__ Key3 load_key(const FlowArgs& p, uint32_t e) {
    const uint4* K = p.keys + 3ull * e;
    return Key3{K[0], K[1], K[2]};
}
__device__ __forceinline__ bool same_key(const Key3& x, const Key3& y) {
    return x.a.x == y.a.x && x.a.y == y.a.y && x.a.z == y.a.z && x.a.w == y.a.w && x.b.x == y.b.x && x.b.y == y.b.y &&
           x.b.z == y.b.z && x.b.w == y.b.w && x.c.x == y.c.x && x.c.y == y.c.y;
}

__global__ __launch_bounds__(256) void flow_elect(FlowArgs p) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x, N = p.n + p.n_known;
    if (e >= N) return;
    const Key3 me = load_key(p, e);
    if (me.c.w == 0u) return;
    const uint32_t mask = p.cap - 1u;
    uint32_t slot = me.c.z & mask;
    for (uint32_t step = 0; step < p.cap; ++step, slot = (slot + 1u) & mask) {
        const uint32_t cur = atomicCAS(&p.table[slot], EMPTY, e);
        if (cur == EMPTY) return;                                   // claimed
        if (cur < N && same_key(me, load_key(p, cur))) {            // the group's slot: keep the smallest entry
            atomicMin(&p.table[slot], e);
            return;
        }
    }
}

__global__ __launch_bounds__(256) void flow_resolve(FlowArgs p) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= p.n) return;
    const uint32_t e = p.n_known + f, N = p.n + p.n_known;
    const Key3 me = load_key(p, e);
    uint32_t leader = EMPTY;
    if (me.c.w != 0u) {
        const uint32_t mask = p.cap - 1u;
        uint32_t slot = me.c.z & mask;
        for (uint32_t step = 0; step < p.cap; ++step, slot = (slot + 1u) & mask) {
            const uint32_t cur = p.table[slot];
            if (cur >= N) break;                                    // a free slot: the frame was never entered
            if (same_key(me, load_key(p, cur))) {
                leader = cur;
                break;
            }
        }
    }
    p.ka[f] = leader;
    p.va[f] = f;
}

// ---------------------------------------------------------------- the stable radix sort

__global__ __launch_bounds__(FLOW_TILE) void radix_hist(const uint32_t* __restrict__ kin, uint32_t n, uint32_t shift,
                                                        uint32_t* __restrict__ hist, uint32_t ntiles) {
    __shared__ uint32_t H[256];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, i = tile * FLOW_TILE + tid;
    if (tid < 256u) H[tid] = 0u;
    __syncthreads();
    if (i < n) atomicAdd(&H[(kin[i] >> shift) & 255u], 1u);
    __syncthreads();
    if (tid < 256u) hist[tid * ntiles + tile] = H[tid];
}

// a[0 .. len) becomes its exclusive prefix sum, in place: ONE workgroup, ceil(len / FLOW_TILE) steps.
__global__ __launch_bounds__(FLOW_TILE) void scan_excl(uint32_t* __restrict__ a, uint32_t len) {
    __shared__ uint32_t W[FLOW_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < len; b += FLOW_TILE) {
        const uint32_t i = b + tid;
        const uint32_t v = i < len ? a[i] : 0u;
        const uint32_t inc = wave_scan_add(v);
        if (lane == 63u) W[wv] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < FLOW_WAVES; ++w) {
            const uint32_t t = W[w];
            before += w < wv ? t : 0u;
            total += t;
        }
        if (i < len) a[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(FLOW_TILE) void radix_scatter(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                           uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                           uint32_t n, uint32_t shift, const uint32_t* __restrict__ offs,
                                                           uint32_t ntiles) {
    __shared__ uint32_t C[FLOW_WAVES][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, tile = blockIdx.x, i = tile * FLOW_TILE + tid;
    const bool in = i < n;
    const uint32_t key = in ? kin[i] : EMPTY, val = in ? vin[i] : 0u;
    const uint32_t digit = (key >> shift) & 255u;
    for (uint32_t j = tid; j < FLOW_WAVES * 256u; j += FLOW_TILE) (&C[0][0])[j] = 0u;
    // the lanes of this wave with my digit: rank among them = my place inside the wave's run of it
    uint64_t m = __builtin_amdgcn_ballot_w64(in);
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
        m &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (in && rank == 0u) C[wv][digit] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    if (tid < 256u) {                   // per digit: each wave's count becomes the count of the waves before it
        uint32_t run = 0;
#pragma unroll
        for (uint32_t w = 0; w < FLOW_WAVES; ++w) {
            const uint32_t t = C[w][tid];
            C[w][tid] = run;
            run += t;
        }
    }
    __syncthreads();
    if (in) {
        const uint32_t pos = offs[digit * ntiles + tile] + C[wv][digit] + rank;
        if (pos < n) {
            kout[pos] = key;
            vout[pos] = val;
        }
    }
}

// ---------------------------------------------------------------- the outputs

// Slot i of the sorted order: head / tail of a run of one leader (selected frames only), and whether
// that leader is a frame (a group behind the table's).
struct Run {
    uint32_t key;
    bool sel, head, tail, own;
};
__device__ __forceinline__ Run run_of(const uint32_t* __restrict__ k, uint32_t i, uint32_t n, uint32_t n_known) {
    Run r{EMPTY, false, false, false, false};
    if (i >= n) return r;
    r.key = k[i];
    r.sel = r.key != EMPTY;
    r.head = r.sel && (i == 0u || k[i - 1u] != r.key);
    r.tail = r.sel && (i + 1u == n || k[i + 1u] != r.key);
    r.own = r.key >= n_known;
    return r;
}

__global__ __launch_bounds__(FLOW_TILE) void flow_heads(const uint32_t* __restrict__ k, uint32_t n, uint32_t n_known,
                                                        uint32_t* __restrict__ cnt) {
    __shared__ uint32_t S;
    const uint32_t tid = threadIdx.x, i = blockIdx.x * FLOW_TILE + tid;
    if (tid == 0u) S = 0u;
    __syncthreads();
    const Run r = run_of(k, i, n, n_known);
    const uint64_t b = __builtin_amdgcn_ballot_w64(r.head && r.own);
    if ((tid & 63u) == 0u && b) atomicAdd(&S, (uint32_t)__builtin_popcountll(b));
    __syncthreads();
    if (tid == 0u) cnt[blockIdx.x] = S;
}

__global__ __launch_bounds__(FLOW_TILE) void flow_emit(FlowArgs p, const uint32_t* __restrict__ k, const uint32_t* __restrict__ v,
                                                       const uint32_t* __restrict__ tile_before) {
    __shared__ uint32_t W[FLOW_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, i = blockIdx.x * FLOW_TILE + tid;
    const Run r = run_of(k, i, p.n, p.n_known);
    const uint32_t flag = (r.head && r.own) ? 1u : 0u;
    const uint32_t inc = wave_scan_add(flag);
    if (lane == 63u) W[wv] = inc;
    __syncthreads();
    uint32_t before = tile_before[blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < FLOW_WAVES; ++w) before += w < wv ? W[w] : 0u;
    const uint32_t heads = before + inc;                // own-leader run heads in slots 0 .. i
    if (i >= p.n) return;
    const uint32_t f = v[i];
    pico_csum_desc_dev od{0, 0, 0};
    if (r.sel && f < p.n) {
        uint64_t off;
        uint32_t avail;
        if (net_region(p, p.desc[f], off, avail)) od = pico_csum_desc_dev{off, avail, 0u};
    }
    p.o_desc[i] = od;
    p.o_index[i] = f;
    const uint32_t g = r.own ? p.n_known + heads - 1u : r.key;
    if (r.sel && g < p.n + p.n_known) {
        if (r.head) p.o_groups[2u * g] = i;
        if (r.tail) p.o_groups[2u * g + 1u] = i + 1u;   // the run's end: flow_counts turns it into a count
    }
    if (i + 1u == p.n) {
        p.o_counts[0] = p.n_known + heads;
        if (r.sel) p.o_counts[1] = p.n;
    }
    if (!r.sel && (i == 0u || k[i - 1u] != EMPTY)) p.o_counts[1] = i;
}

__global__ __launch_bounds__(256) void flow_counts(uint32_t* __restrict__ groups, uint32_t N) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= N) return;
    const uint32_t end = groups[2u * g + 1u];
    if (end) groups[2u * g + 1u] = end - groups[2u * g];
}

}  // namespace

extern "C" {

// lay[]: the byte offsets in `scratch` of keys, table, ka, va, kb, vb, hist (pico_csum.c: flow_layout).
int pico_csum_launch_flow_group(const void* base, uint64_t base_len, const void* desc, uint32_t n, const uint8_t* verdict_in,
                                uint32_t mode_flags, const void* known, uint32_t n_known, uint32_t seed, void* o_desc,
                                uint32_t* o_index, uint32_t* o_groups, uint32_t* o_counts, void* scratch,
                                const uint64_t* lay, uint32_t cap, uint32_t ntiles, uint32_t passes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* sc = static_cast<uint8_t*>(scratch);
    const uint32_t N = n + n_known;
    FlowArgs a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(desc), n, verdict_in,
               mode_flags & 0xFu, (mode_flags & MF_ETH) ? 1u : 0u, static_cast<const uint8_t*>(known), n_known, seed,
               static_cast<pico_csum_desc_dev*>(o_desc), o_index, o_groups, o_counts,
               reinterpret_cast<uint4*>(sc + lay[0]), reinterpret_cast<uint32_t*>(sc + lay[1]), cap,
               reinterpret_cast<uint32_t*>(sc + lay[2]), reinterpret_cast<uint32_t*>(sc + lay[3]),
               reinterpret_cast<uint32_t*>(sc + lay[4]), reinterpret_cast<uint32_t*>(sc + lay[5]),
               reinterpret_cast<uint32_t*>(sc + lay[6]), ntiles};
    hipError_t e;
    if ((e = hipMemsetAsync(a.table, 0xFF, 4ull * cap, s)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(o_groups, 0, 8ull * N, s)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(o_counts, 0, 8u, s)) != hipSuccess) return (int)e;
    const dim3 gN((N + 255u) / 256u), gn((n + 255u) / 256u), gt(ntiles);
    hipLaunchKernelGGL(flow_parse, gN, dim3(256), 0, s, a);
    hipLaunchKernelGGL(flow_elect, gN, dim3(256), 0, s, a);
    hipLaunchKernelGGL(flow_resolve, gn, dim3(256), 0, s, a);
    uint32_t *ki = a.ka, *vi = a.va, *ko = a.kb, *vo = a.vb;
    for (uint32_t ps = 0; ps < passes; ++ps) {
        hipLaunchKernelGGL(radix_hist, gt, dim3(FLOW_TILE), 0, s, ki, n, 8u * ps, a.hist, ntiles);
        hipLaunchKernelGGL(scan_excl, dim3(1), dim3(FLOW_TILE), 0, s, a.hist, 256u * ntiles);
        hipLaunchKernelGGL(radix_scatter, gt, dim3(FLOW_TILE), 0, s, ki, vi, ko, vo, n, 8u * ps, a.hist, ntiles);
        uint32_t* t = ki; ki = ko; ko = t;
        t = vi; vi = vo; vo = t;
    }
    hipLaunchKernelGGL(flow_heads, gt, dim3(FLOW_TILE), 0, s, ki, n, n_known, a.hist);
    hipLaunchKernelGGL(scan_excl, dim3(1), dim3(FLOW_TILE), 0, s, a.hist, ntiles);
    hipLaunchKernelGGL(flow_emit, gt, dim3(FLOW_TILE), 0, s, a, ki, vi, a.hist);
    hipLaunchKernelGGL(flow_counts, gN, dim3(256), 0, s, o_groups, N);
    return (int)hipGetLastError();
}

}  // extern "C"
