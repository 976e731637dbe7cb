// pico_csum_k_tcprx.hip -- TCP receive coalescing (what a NIC calls LRO / GRO): a connection's
// received segments verified and their in-order byte stream delivered into one contiguous region,
// in one pass that reads each delivered payload byte once -- and its launcher.  The inverse of the
// send segmentation (pico_csum_k_tcpseg.hip), whose per-segment sums it keeps, and the TCP sibling
// of the reassembly gather (pico_csum_k_frag.hip).  Helpers, the IPv4 header rules (ipv4_classify),
// the segment parse (seg_parse, shared with pico_csum_k_tcpack.hip), the 16-byte unit mover
// (unit_pair_move) and the arithmetic contract: pico_csum_dev.h.  The contract:
// include/pico_csum.h, pico_tcp_coalesce_batch_dev.
//
// Reference: pico_transport_crc_check (stack/pico_socket.c:1916-1968), pico_tcp_input /
// tcp_action_by_flags (modules/pico_tcp.c:2787-2867), tcp_data_in (:1717-1776: an in-order segment
// is enqueued and rcv_nxt scrolls over what is queued behind it, :1677-1683; a segment ahead of
// rcv_nxt is queued with SACK and dropped without, :1693-1714; one behind it is dropped, :1687),
// segment_from_frame (:97-119: a copy of the payload) and pico_tcp_read (:1149-1182: a second copy).
//
// One workgroup per connection:
//   1. every thread parses segment headers into LDS (seg_parse): the network header's rules, the
//      IPv4 header checksum on the spot, the TCP flags, seq and payload length, and the word sum of
//      the pseudo header and the TCP header -- the gather then only adds payload;
//   2. wave 0 plans the chain (plan_chain): the prefix of the group that arrived in order by a prefix
//      scan per 64 arrivals; then, from cur = its end, a ballot for seq == cur over the candidates, 64
//      a round, takes the earliest arrival (without SACK: behind the last taken one), until none
//      matches or the next one does not fit the region;
//   3. all waves gather the chain's members two at a time, wave w the pairs w, w + 4, ..., through
//      unit_pair_move: a member's place in the region follows from its seq alone, whole units are
//      stored non-temporally, each member's readable block ends with its own segment's buffer, and
//      every unit's bytes enter its OWN member's sum, two accumulators and two DPP reductions per pair;
//   4. a member whose sum fails is struck (L4_BAD); if any was, wave 0 plans again without them and
//      the new chain is gathered IN FULL: a placement depends on seq alone, but between two rounds a
//      struck chain's later members may have been copied over a place the final chain fills from a
//      member gathered before them, so a round that copied only its new members could leave another
//      segment's bytes inside [0, out_len) when overlapping segments disagree.  Rounds past the first
//      happen only on a corrupted segment.
// No library scratch, one launch, graph-capturable.  The per-connection results are written by
// vector stores from one lane.
#include "pico_csum_dev.h"

namespace {

constexpr uint32_t TCPRX_MAX = 512u;        // segments per connection handled on device
// Launch shapes, the send segmentation's two (the thresholds: SHORT_GROUPS_MIN / SHORT_SLOTS_AVG,
// pico_csum_dev.h): four waves per connection; large batches of short groups one wave per
// connection -- there four waves would share two to four pairs.  Measured at ONE point, 29360
// connections of 7 segments (profiles/tcprx/ab_shapes.txt).
constexpr uint32_t TRX_U = 3u;              // 64-unit rows per gather step: two 1448-byte payloads

struct TcpRxArgs {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* seg;      // received frames (off -> network header, len = bytes available)
    uint32_t n_seg;
    const uint32_t* grp;                // 2 per connection: first segment, count (arrival order)
    const uint32_t* conn;               // 2 per connection: rcv_nxt, cflags (bit 0: sack_ok)
    uint32_t n_conn;
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;    // per connection: output region (off, capacity)
    uint32_t* o_len;
    uint8_t* seg_verdict;
    uint8_t* verdict;
};

struct TcpRxLds {
    uint32_t seq[TCPRX_MAX];
    uint32_t hsum[TCPRX_MAX];   // word sum of the pseudo header and the TCP header
    uint16_t pl[TCPRX_MAX];     // payload bytes
    uint16_t mark[TCPRX_MAX];   // the last round that had the segment on its chain
    uint16_t ord[TCPRX_MAX];    // chain position -> segment
    uint64_t src[TCPRX_MAX];    // the payload's address (no descriptor re-read in the gather)
    uint16_t trail[TCPRX_MAX];  // the buffer's bytes behind the payload (clamped: only the last-unit rule reads it)
    uint8_t st[TCPRX_MAX];      // 0: a candidate for the chain; else the segment's verdict
    uint32_t nchain, end, anybad;
};

// Wave 0: the chain over the candidates not struck, into L.ord / L.nchain / L.end; its members get
// mark = round.
__device__ __forceinline__ void plan_chain(TcpRxLds& L, uint32_t cnt, uint32_t rcv_nxt, bool sack, uint32_t cap,
                                           uint32_t round, uint32_t lane) {
    uint32_t cur = rcv_nxt, n = 0, start = 0;          // start: without SACK, behind the last taken arrival
    // the common case, a prefix of the group that arrived in order: arrival j is the chain's member j
    // when every arrival before it is one and its seq is rcv_nxt + their payloads (it is then the
    // earliest arrival with that seq: every earlier one's is smaller) -- a prefix scan per 64 arrivals
    // in place of a ballot step per member
    for (uint32_t j0 = 0; j0 < cnt; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const bool cand = j < cnt && L.st[j] == 0u;
        const uint32_t pl = cand ? L.pl[j] : 0u;
        const uint32_t rel = (cur - rcv_nxt) + wave_scan_add(pl) - pl;
        const bool ok = cand && L.seq[j] == rcv_nxt + rel && (uint64_t)rel + pl <= cap;
        const uint64_t fail = __builtin_amdgcn_ballot_w64(!ok);
        const uint32_t k = fail ? (uint32_t)__builtin_ctzll(fail) : 64u;
        if (lane < k) {
            L.ord[n + lane] = (uint16_t)j;
            L.mark[j] = (uint16_t)round;
        }
        if (k) cur = rcv_nxt + (uint32_t)__builtin_amdgcn_readlane((int)(rel + pl), (int)(k - 1u));
        n += k;
        if (k < 64u) break;
    }
    if (!sack) start = n;
    // the rest: a ballot for seq == cur per member
    while (n < cnt) {
        uint32_t hit = NONE;
        for (uint32_t j0 = start & ~63u; j0 < cnt && hit == NONE; j0 += 64u) {
            const uint32_t j = j0 + lane;
            const bool m = j < cnt && j >= start && L.st[j] == 0u && L.seq[j] == cur;
            const uint64_t b = __builtin_amdgcn_ballot_w64(m);
            if (b) hit = j0 + (uint32_t)__builtin_ctzll(b);
        }
        if (hit == NONE) break;
        const uint32_t pl = L.pl[hit];
        if ((uint64_t)(cur - rcv_nxt) + pl > cap) break;                // the region is the window
        if (lane == 0) {
            L.ord[n] = (uint16_t)hit;
            L.mark[hit] = (uint16_t)round;
        }
        ++n;
        cur += pl;
        if (!sack) start = hit + 1u;
    }
    if (lane == 0) {
        L.nchain = n;
        L.end = cur;
    }
}

template <uint32_t TRX_WAVES>
__global__ __launch_bounds__(64 * TRX_WAVES) void tcp_coalesce_kernel(TcpRxArgs p) {
    __shared__ TcpRxLds L;
    constexpr uint32_t NT = 64u * TRX_WAVES;
    const uint32_t g = blockIdx.x;
    if (g >= p.n_conn) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t first = p.grp[2 * g], cnt = p.grp[2 * g + 1];
    const uint32_t rcv_nxt = p.conn[2 * g], cflags = p.conn[2 * g + 1];
    const pico_csum_desc_dev od = p.odesc[g];
    const bool sack = (cflags & 1u) != 0u;
    const uint32_t cap = od.len;

    // ---- the connection's own checks (workgroup-uniform): nothing of the region is written
    const bool grp_in = slots_in(first, cnt, p.n_seg);
    const bool bad = cnt == 0u || cnt > TCPRX_MAX || !grp_in || span_out(od, p.out_len) || (cflags & ~1u) != 0u;
    if (bad) {
        if (p.seg_verdict && grp_in)
            for (uint32_t j = tid; j < cnt; j += NT) p.seg_verdict[first + j] = (uint8_t)V_MALFORMED;
        if (tid == 0) {
            if (p.o_len) p.o_len[g] = 0u;
            if (p.verdict) p.verdict[g] = (uint8_t)V_MALFORMED;
        }
        return;
    }

    // ---- 1. parse
    for (uint32_t j = tid; j < cnt; j += NT) {
        const pico_csum_desc_dev d = p.seg[first + j];
        uint32_t seq, pl, poff, hsum;
        const uint32_t st = seg_parse(p, d, seq, pl, poff, hsum);
        L.seq[j] = seq;
        L.hsum[j] = hsum;
        L.pl[j] = (uint16_t)pl;
        L.mark[j] = 0;
        L.src[j] = reinterpret_cast<uint64_t>(p.base) + d.off + poff;
        L.trail[j] = (uint16_t)min(d.len - min(d.len, poff + pl), 0xFFFFu);
        L.st[j] = (uint8_t)st;
    }
    __syncthreads();

    const uint64_t D = reinterpret_cast<uint64_t>(p.out) + od.off;          // the stream's byte 0
    uint32_t round = 0;
    for (;;) {
        ++round;
        // ---- 2. the chain
        if (wv == 0) {
            if (lane == 0) L.anybad = 0u;
            plan_chain(L, cnt, rcv_nxt, sack, cap, round, lane);
        }
        __syncthreads();

        // ---- 3. gather + per-member sums
        const uint32_t nchain = L.nchain, npair = (nchain + 1u) >> 1;
        for (uint32_t jp = wv; jp < npair; jp += TRX_WAVES) {
            const bool hasB = 2u * jp + 1u < nchain;
            const uint32_t iA = uni(L.ord[2u * jp]), iB = hasB ? uni(L.ord[2u * jp + 1u]) : iA;
            const uint32_t plA = uni(L.pl[iA]), plB = hasB ? uni(L.pl[iB]) : 0u;
            const uint64_t sA = uni64(L.src[iA]), sB = uni64(L.src[iB]);                                 // the payloads
            // the end of the last 16-byte block that overlaps each segment's buffer (or an earlier block's,
            // where more than 65535 bytes lie behind the payload)
            const uint64_t eA = (sA + plA + uni(L.trail[iA]) + 15u) & ~(uint64_t)15;
            const uint64_t eB = (sB + uni(L.pl[iB]) + uni(L.trail[iB]) + 15u) & ~(uint64_t)15;
            const uint64_t dA = uni64(D + (uint32_t)(L.seq[iA] - rcv_nxt)), dB = uni64(D + (uint32_t)(L.seq[iB] - rcv_nxt));

            uint32_t accA = 0, accB = 0;
            unit_pair_move<TRX_U, true, true>(sA, sB, dA, dB, eA, eB, plA, plB, hasB, lane, accA, accB);
            const uint32_t payA = wave_total(accA);
            const uint32_t payB = wave_total(accB);
            // ---- 4. pico_tcp_checksum over what was copied: a member that fails is struck
            if (lane == 0) {
                if (finalize(L.hsum[iA] + payA) != 0u) {
                    L.st[iA] = (uint8_t)V_L4_BAD;
                    L.anybad = 1u;
                }
                if (hasB && finalize(L.hsum[iB] + payB) != 0u) {
                    L.st[iB] = (uint8_t)V_L4_BAD;
                    L.anybad = 1u;
                }
            }
        }
        __syncthreads();
        const uint32_t again = L.anybad;
        __syncthreads();                                // (wave 0 clears it for the next round)
        if (!again) break;
    }

    // ---- the verdicts, with the chain's end final
    const uint32_t E = L.end;
    if (p.seg_verdict) {
        for (uint32_t j = tid; j < cnt; j += NT) {
            uint32_t v = L.st[j];
            if (v == 0u) v = L.mark[j] == round ? V_ACCEPT : (seq_before(L.seq[j], E) ? V_TCP_OLD : V_TCP_HELD);
            p.seg_verdict[first + j] = (uint8_t)v;
        }
    }
    if (tid == 0) {
        if (p.o_len) p.o_len[g] = E - rcv_nxt;
        if (p.verdict) p.verdict[g] = (uint8_t)V_ACCEPT;
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_tcp_coalesce(const void* base, uint64_t base_len, const void* seg, uint32_t n_seg,
                                  const uint32_t* groups, const uint32_t* conn, uint32_t n_conn, void* out, uint64_t out_len,
                                  const void* out_desc, uint32_t* o_len, uint8_t* seg_verdict, uint8_t* verdict,
                                  void* stream) {
    if (n_conn == 0) return (int)hipSuccess;
    TcpRxArgs a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(seg), n_seg, groups,
                conn, n_conn, static_cast<uint8_t*>(out), out_len, static_cast<const pico_csum_desc_dev*>(out_desc),
                o_len, seg_verdict, verdict};
    if (short_groups(n_conn, n_seg))
        hipLaunchKernelGGL(tcp_coalesce_kernel<1u>, dim3(n_conn), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(tcp_coalesce_kernel<4u>, dim3(n_conn), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
