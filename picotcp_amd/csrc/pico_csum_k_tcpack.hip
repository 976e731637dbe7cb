// pico_csum_k_tcpack.hip -- the burst's ACKs: one launch behind the TCP receive coalescing
// (pico_csum_k_tcprx.hip) that finishes the checksum verdicts the coalescing left open (TCP_OLD and
// TCP_HELD segments: "payload not read"), and writes each connection's ready-to-send ACK frame --
// ack number, window, options with the SACK blocks of the held segments, both checksums -- and its
// launcher.  Helpers, the segment parse (seg_parse), the header word's halves and store (halves,
// store_word) and the arithmetic contract: pico_csum_dev.h.
// The contract: include/pico_csum.h, pico_tcp_ack_batch_dev.
//
// Reference: tcp_data_in_send_ack -> tcp_send_ack -> tcp_send_empty (modules/pico_tcp.c:1716-1725,
// :1324-1327, :1286-1322), tcp_sack_prepare (:1597-1657), tcp_options_size (:703-731),
// tcp_add_options / tcp_add_sack_option (:582-617, :560-580), tcp_set_space (:681-700),
// pico_ipv4_frame_push (modules/pico_ipv4.c:1039-1079).
//
// One workgroup per connection:
//   1. every thread reads segment verdicts; a TCP_OLD / TCP_HELD one is parsed into LDS (seg_parse:
//      seq, payload, the pseudo header's and the TCP header's word sum) and put on the sum list;
//   2. the waves sum the listed payloads two at a time (pair_sum): aligned 16-byte blocks, edge bytes
//      masked, the pairing relative to each payload's own start; checksum only, nothing is stored.
//      The blocks are the aligned ones that overlap the payload, which lies inside its segment's
//      buffer: the whole-block read rule covers them and nothing behind them is read;
//   3. the queue: the verified TCP_HELD segments (with sack_ok), the later arrival of an equal seq
//      dropped, ranked by seq - rcv' -- a count-smaller rank per segment over LDS, bounded by the
//      group's size;
//   4. one lane walks the ranked queue through tcp_sack_prepare (with the reference's own
//      next_segment: one contiguous run), computes the window and lays the
//      frame out in LDS over the template's words;
//   5. wave 0 takes the frame's words into registers, sums both headers there (wave_total), sets the
//      two crc fields and stores the words (store_word).
// No library scratch, one launch, graph-capturable.  Every loop is bounded by the group's size.
#include "pico_csum_dev.h"

namespace {

constexpr uint32_t TCPACK_MAX = 512u;       // segments per connection (the coalescing's limit)
constexpr uint32_t TAK_U = 3u;              // 64-block rows per sum step: two 1460-byte payloads at any alignment

// struct pico_csum_tcp_ack (include/pico_csum.h), 16 bytes
struct pico_csum_tcp_ack_dev {
    uint32_t space, tsval, tsecr, aflags;
};

struct TcpAckArgs {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* seg;
    uint32_t n_seg;
    const uint32_t* grp;                // 2 per connection: first segment, count
    const uint32_t* conn;               // 2 per connection: rcv_nxt, cflags (bit 0: sack_ok)
    uint32_t n_conn;
    const uint32_t* o_len;              // the coalescing's out_len
    uint8_t* seg_verdict;               // the coalescing's verdicts, updated in place
    const uint8_t* tmpl;
    uint64_t tmpl_len;
    const pico_csum_desc_dev* tdesc;    // per connection: the header template
    const pico_csum_tcp_ack_dev* ack;
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;    // per connection: the frame's region
    pico_csum_desc_dev* o_ack;
    uint8_t* verdict;
};

// per-segment state bits
constexpr uint32_t S_SUM = 1u, S_HELD = 2u, S_BAD = 4u, S_QUEUED = 8u;

struct TcpAckLds {
    uint64_t src[TCPACK_MAX];       // the payload's address
    uint32_t seq[TCPACK_MAX];
    uint32_t hsum[TCPACK_MAX];      // word sum of the pseudo header and the TCP header
    uint16_t pl[TCPACK_MAX];        // payload bytes
    uint16_t list[TCPACK_MAX];      // the segments to sum
    uint16_t ranked[TCPACK_MAX];    // queue position -> segment
    uint8_t st[TCPACK_MAX];
    uint32_t frame[25];             // the ACK: 40 + 60 bytes at most
    uint32_t nlist, due, nqueue, held, flen, malformed;
};

// One wave sums the payloads of two segments A and B -- pl bytes at address s, any alignment each --
// without storing anything.  A payload that starts r = s & 15 bytes into a 16-byte block has blocks
// [0, (r + pl + 15) / 16), one aligned 16-byte load each; the two payloads' blocks share one index
// space, A's first, U rows of 64 blocks a step with all loads issued before the first sum.  The
// payload's bytes of a block are selected by mask, and for an odd r the bytes of each 16-bit half
// are swapped first (SEL_ODD), so the pairing is relative to the payload's own start.  hasB false:
// plB and sB are not used.  All arguments but lane are wave-uniform.
template <uint32_t U>
__device__ __forceinline__ void pair_sum(uint64_t sA, uint64_t sB, uint32_t plA, uint32_t plB, bool hasB, uint32_t lane,
                                         uint32_t& accA, uint32_t& accB) {
    const uint32_t rA = (uint32_t)sA & 15u, rB = (uint32_t)sB & 15u;
    const uint32_t nA = (rA + plA + 15u) >> 4, nB = hasB ? (rB + plB + 15u) >> 4 : 0u, nt = nA + nB;
    const uint8_t* a0A = reinterpret_cast<const uint8_t*>(sA - rA);
    const uint8_t* a0B = reinterpret_cast<const uint8_t*>(sB - rB);
    for (uint32_t x0 = 0; x0 < nt; x0 += 64u * U) {
        uint4 c[U];
        uint32_t k[U];
        bool inb[U];
#pragma unroll
        for (uint32_t q = 0; q < U; ++q) {
            const uint32_t x = x0 + 64u * q + lane;
            inb[q] = x >= nA;
            k[q] = inb[q] ? x - nA : x;
            c[q] = make_uint4(0, 0, 0, 0);
            if (x < nt) c[q] = load_chunk(inb[q] ? a0B : a0A, k[q]);
        }
#pragma unroll
        for (uint32_t q = 0; q < U; ++q) {
            const bool live = x0 + 64u * q + lane < nt;
            const uint32_t r = inb[q] ? rB : rA, pl = inb[q] ? plB : plA;
            const uint32_t s = masked_chunk_sum<true>(c[q], 16u * k[q], r, live ? r + pl : 0u, (r & 1u) ? SEL_ODD : SEL_EVEN);
            accA += inb[q] ? 0u : s;
            accB += inb[q] ? s : 0u;
        }
    }
}

// big-endian bytes of v at p (LDS)
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

template <uint32_t TAK_WAVES>
__global__ __launch_bounds__(64 * TAK_WAVES) void tcp_ack_kernel(TcpAckArgs p) {
    __shared__ TcpAckLds L;
    constexpr uint32_t NT = 64u * TAK_WAVES;
    const uint32_t g = blockIdx.x;
    if (g >= p.n_conn) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t first = p.grp[2 * g], cnt = p.grp[2 * g + 1];
    const uint32_t rcv_nxt = p.conn[2 * g], cflags = p.conn[2 * g + 1];
    const pico_csum_desc_dev td = p.tdesc[g], od = p.odesc[g];
    const pico_csum_tcp_ack_dev ak = p.ack[g];
    const bool sack = (cflags & 1u) != 0u, ts_ok = (ak.aflags & 1u) != 0u;

    // ---- the connection's own checks (workgroup-uniform, in an order that never reads past the
    // template's len): nothing is written for a connection that fails one
    const auto reject = [&] {                                               // zero descriptor + MALFORMED
        if (tid == 0) {
            if (p.o_ack) p.o_ack[g] = pico_csum_desc_dev{0, 0, 0};
            if (p.verdict) p.verdict[g] = (uint8_t)V_MALFORMED;
        }
    };
    bool bad = cnt == 0u || cnt > TCPACK_MAX || !slots_in(first, cnt, p.n_seg) || (cflags & ~1u) != 0u || (ak.aflags & ~1u) != 0u;
    bad = bad || span_out(td, p.tmpl_len) || td.len < 1u;
    const uint8_t* h = p.tmpl + td.off;
    uint32_t N = 20u;
    bool v6 = false;
    if (!bad) {
        const uint32_t b0 = h[0];
        v6 = (b0 >> 4) == 6u;
        N = v6 ? 40u : 20u;
        bad = !(v6 || (b0 >> 4) == 4u) || td.len < N;
        if (!bad) bad = v6 ? (uint32_t)h[6] != 6u : ((b0 & 15u) != 5u || (uint32_t)h[9] != 6u);
        bad = bad || td.len < N + 20u;
    }
    if (bad || span_out(od, p.out_len)) return reject();
    const uint32_t rcv = rcv_nxt + p.o_len[g];                              // rcv'

    if (tid == 0) L.nlist = L.due = L.nqueue = L.held = L.flen = L.malformed = 0u;
    __syncthreads();

    // ---- 1. the verdicts as they came; the OLD / HELD segments' parse
    uint32_t due = 0;
    for (uint32_t j = tid; j < cnt; j += NT) {
        const uint32_t v = p.seg_verdict[first + j];
        uint32_t st = 0;
        if (v == V_TCP_OLD || v == V_TCP_HELD) {
            const pico_csum_desc_dev d = p.seg[first + j];
            uint32_t seq, pl, poff, hsum;
            // (a segment that does not parse as data did not get this verdict from the coalescing: it
            // is left alone and counts for nothing)
            if (seg_parse(p, d, seq, pl, poff, hsum) == 0u) {
                st = S_SUM | (v == V_TCP_HELD ? S_HELD : 0u);
                L.seq[j] = seq;
                L.hsum[j] = hsum;
                L.pl[j] = (uint16_t)pl;
                L.src[j] = reinterpret_cast<uint64_t>(p.base) + d.off + poff;
                L.list[atomicAdd(&L.nlist, 1u)] = (uint16_t)j;
            }
        } else if (v == V_ACCEPT) {
            due = 1u;
        }
        L.st[j] = (uint8_t)st;
    }
    if (due) L.due = 1u;
    __syncthreads();

    // ---- 2. pico_tcp_checksum of the listed segments, a pair per wave
    const uint32_t nlist = L.nlist, npair = (nlist + 1u) >> 1;
    for (uint32_t jp = wv; jp < npair; jp += TAK_WAVES) {
        const bool hasB = 2u * jp + 1u < nlist;
        const uint32_t iA = uni(L.list[2u * jp]), iB = hasB ? uni(L.list[2u * jp + 1u]) : iA;
        uint32_t accA = 0, accB = 0;
        pair_sum<TAK_U>(uni64(L.src[iA]), uni64(L.src[iB]), uni(L.pl[iA]), uni(L.pl[iB]), hasB, lane, accA, accB);
        const uint32_t payA = wave_total(accA);
        const uint32_t payB = wave_total(accB);
        if (lane == 0) {
            if (finalize(L.hsum[iA] + payA) != 0u) L.st[iA] |= (uint8_t)S_BAD;
            else L.due = 1u;
            if (hasB) {
                if (finalize(L.hsum[iB] + payB) != 0u) L.st[iB] |= (uint8_t)S_BAD;
                else L.due = 1u;
            }
        }
    }
    __syncthreads();

    // ---- 3. the queue: verified held segments, unique by seq with the earliest arrival kept
    // (pico_tree_insert refuses the later one); without sack_ok the reference drops them (:1696)
    const uint32_t QMASK = S_SUM | S_HELD | S_BAD, QVAL = S_SUM | S_HELD;
    if (sack) {
        for (uint32_t j = tid; j < cnt; j += NT) {
            if ((L.st[j] & QMASK) != QVAL) continue;
            bool dup = false;
            for (uint32_t k = 0; k < j; ++k) dup = dup || ((L.st[k] & QMASK) == QVAL && L.seq[k] == L.seq[j]);
            if (!dup) {
                L.st[j] |= (uint8_t)S_QUEUED;
                atomicAdd(&L.held, (uint32_t)L.pl[j]);
                atomicAdd(&L.nqueue, 1u);
            }
        }
    }
    __syncthreads();
    // its order: ascending seq - rcv'.  A held segment lies at or beyond rcv', at most 2^31 ahead, so
    // this is pico_seq_compare's order, and it is a total order whatever the verdicts were.
    if (L.nqueue) {
        for (uint32_t j = tid; j < cnt; j += NT) {
            if (!(L.st[j] & S_QUEUED)) continue;
            const uint32_t dj = L.seq[j] - rcv;
            uint32_t rank = 0;
            for (uint32_t k = 0; k < cnt; ++k) rank += ((L.st[k] & S_QUEUED) && L.seq[k] - rcv < dj) ? 1u : 0u;
            L.ranked[rank] = (uint16_t)j;
        }
    }
    __syncthreads();

    // ---- the template's N + 20 bytes into the frame (wave 0; word l in lane l)
    const uint32_t tw0 = N >> 2;
    if (wv == 0 && lane < tw0 + 5u) L.frame[lane] = ld32(h + 4u * lane);
    __syncthreads();

    // ---- 4. one lane: the blocks, the window, the frame's fields and options
    if (tid == 0 && L.due) {
        // tcp_sack_prepare (:1597-1657) restated literally over the queue and rcv', with its own
        // first_segment / next_segment (:161-179).  Its quirks, kept and not repaired:
        //   * next_segment is NOT the tree's successor: it is peek_segment(seq + payload_len), the
        //     segment that starts exactly where this one ends, or none.  So the walk follows ONE
        //     contiguous run from the queue's first segment and ends at its first gap: in practice at
        //     most one block, the run of the lowest held segment; later runs are never reported;
        //   * at most 3 blocks; each is pushed to the FRONT of t->sacks, so they would be emitted
        //     highest-first;
        //   * the segment that breaks a run closes the open block and is itself skipped (with this
        //     next_segment `pkt->seq == right` always holds: the branch is kept as it stands);
        //   * left == 0 means "no open block": a run that starts at seq 0 loses its first segment
        //     (the next one overwrites it) or, alone, the whole block;
        //   * `pkt->seq < rcv_nxt` is a raw compare: past a 2^32 wrap of the stream a held segment's
        //     seq is below rcv' and it is skipped.
        // The queue is ranked by seq - rcv', so the segment at seq + payload_len, if any, lies ahead
        // of the current one: the search only moves forward, the whole walk is one pass.
        uint32_t blk[3][2];
        uint32_t nb = 0, left = 0, right = 0;
        const uint32_t nq = L.nqueue;
        uint32_t i = nq ? 0u : NONE;                                        // first_segment
        while (nb < 3u) {
            if (i == NONE) {
                if (left) {
                    blk[nb][0] = left;
                    blk[nb][1] = right;
                    ++nb;
                }
                break;
            }
            const uint32_t j = L.ranked[i], s = L.seq[j], pl = L.pl[j];
            {                                                               // pkt = next_segment(pkt)
                const uint32_t t = s + pl, dt = t - rcv;
                uint32_t k = i + 1u;
                while (k < nq && L.seq[L.ranked[k]] - rcv < dt) ++k;
                i = k < nq && L.seq[L.ranked[k]] == t ? k : NONE;
            }
            if (s < rcv) continue;
            if (!left) {
                left = s;
                right = s + pl;
                continue;
            }
            if (s == right) {
                right += pl;
                continue;
            }
            blk[nb][0] = left;
            blk[nb][1] = right;
            ++nb;
            left = right = 0;
        }
        // tcp_set_space (:681-700): the queue's size is what the chain delivered plus the held bytes
        const int64_t sp = (int64_t)ak.space - (int64_t)p.o_len[g] - (int64_t)L.held;
        uint32_t space = sp < 0 ? 0u : (uint32_t)sp, shift = 0;
        while (space > 0xFFFFu) {
            space >>= 1;
            ++shift;
        }
        // tcp_options_size (:703-731): WS, timestamps, END, the SACK option; a multiple of 4
        const uint32_t optsz = (3u + (ts_ok ? 10u : 0u) + 1u + (nb ? 2u + 8u * nb : 0u) + 3u) & ~3u;
        const uint32_t thl = 20u + optsz;
        uint8_t* f = reinterpret_cast<uint8_t*>(L.frame);
        if (v6) {
            f[4] = (uint8_t)(thl >> 8);
            f[5] = (uint8_t)thl;
        } else {
            f[2] = (uint8_t)((20u + thl) >> 8);
            f[3] = (uint8_t)(20u + thl);
            f[6] = 0x40;                                                    // frag = 40 00
            f[7] = 0;
            f[10] = f[11] = 0;
        }
        uint8_t* t = f + N;
        put_be32(t + 8, rcv);
        t[12] = (uint8_t)((thl << 2) | (t[12] & 0x0Fu));                    // hdr->len = thl << 2 | jumbo
        t[13] = 0x10;
        t[14] = (uint8_t)(space >> 8);
        t[15] = (uint8_t)space;
        t[16] = t[17] = 0;
        // tcp_add_options (:582-617): NOOP fill, WS, timestamps, SACK, END in the last byte
        uint8_t* o = t + 20;
        for (uint32_t k = 0; k < optsz; ++k) o[k] = 1;
        uint32_t ii = 0;
        o[ii++] = 3;
        o[ii++] = 3;
        o[ii++] = (uint8_t)shift;
        if (ts_ok) {
            o[ii++] = 8;
            o[ii++] = 10;
            put_be32(o + ii, ak.tsval);
            put_be32(o + ii + 4, ak.tsecr);
            ii += 8;
        }
        if (nb) {
            o[ii++] = 5;
            o[ii++] = (uint8_t)(2u + 8u * nb);
            for (uint32_t b = nb; b-- > 0u;) {                              // the last pushed block first
                put_be32(o + ii, blk[b][0]);
                put_be32(o + ii + 4, blk[b][1]);
                ii += 8;
            }
        }
        if (ii < optsz) o[optsz - 1u] = 0;
        L.flen = N + thl;
        if (N + thl > od.len) L.malformed = 1u;                            // the region is smaller than the frame
    }
    __syncthreads();

    const uint32_t flen = L.flen;
    if (L.malformed) return reject();

    // ---- the verdicts the coalescing left open
    for (uint32_t j = tid; j < cnt; j += NT)
        if (L.st[j] & S_BAD) p.seg_verdict[first + j] = (uint8_t)V_L4_BAD;
    if (tid == 0) {
        if (p.o_ack) p.o_ack[g] = flen ? pico_csum_desc_dev{od.off, flen, 0} : pico_csum_desc_dev{0, 0, 0};
        if (p.verdict) p.verdict[g] = (uint8_t)V_ACCEPT;
    }

    // ---- 5. the frame: sums from registers, then the stores
    if (wv == 0 && flen) {
        const uint32_t nw = flen >> 2, thl = flen - N;
        const uint32_t w = lane < nw ? L.frame[lane] : 0u;
        const uint32_t j = lane - tw0;                                      // the word's place in the TCP header
        const uint32_t n_part = !v6 && lane < 5u ? halves(w) : 0u;
        const uint32_t a_part = (v6 ? lane >= 2u && lane < 10u : lane >= 3u && lane < 5u) ? halves(w) : 0u;
        const uint32_t t_part = lane >= tw0 && lane < nw ? halves(w) : 0u;
        const uint32_t ncrc = finalize(wave_total(n_part));
        // struct pico_ipv4_pseudo_hdr / pico_ipv6_pseudo_hdr as LE words: the addresses, proto 6, the length
        const uint32_t tcrc = finalize(wave_total(a_part + t_part) + (6u << 8) + bswap16(thl));
        uint32_t v = w;
        if (!v6 && lane == 2u) v = (v & 0xFFFFu) | (bswap16(ncrc) << 16);
        if (j == 4u) v = (v & 0xFFFF0000u) | bswap16(tcrc);
        if (lane < nw) store_word(p.out + od.off + 4u * lane, v);
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_tcp_ack(const void* base, uint64_t base_len, const void* seg, uint32_t n_seg, const uint32_t* groups,
                             const uint32_t* conn, uint32_t n_conn, const uint32_t* o_len, uint8_t* seg_verdict,
                             const void* tmpl, uint64_t tmpl_len, const void* tmpl_desc, const void* ack, void* out,
                             uint64_t out_len, const void* out_desc, void* o_ack, uint8_t* verdict, void* stream) {
    if (n_conn == 0) return (int)hipSuccess;
    TcpAckArgs a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(seg), n_seg, groups,
                 conn, n_conn, o_len, seg_verdict, static_cast<const uint8_t*>(tmpl), tmpl_len,
                 static_cast<const pico_csum_desc_dev*>(tmpl_desc), static_cast<const pico_csum_tcp_ack_dev*>(ack),
                 static_cast<uint8_t*>(out), out_len, static_cast<const pico_csum_desc_dev*>(out_desc),
                 static_cast<pico_csum_desc_dev*>(o_ack), verdict};
    if (short_groups(n_conn, n_seg))
        hipLaunchKernelGGL(tcp_ack_kernel<1u>, dim3(n_conn), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(tcp_ack_kernel<4u>, dim3(n_conn), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
