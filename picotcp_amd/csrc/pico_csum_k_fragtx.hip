// pico_csum_k_fragtx.hip -- IPv4 TX fragmentation scatter fused with the header checksum of every
// fragment and the transport checksum of the whole datagram, and its launcher: the inverse of the
// reassembly gather (pico_csum_k_frag.hip).  Helpers and the arithmetic contract: pico_csum_dev.h.
//
// Reference: pico_socket_xmit_fragments (stack/pico_socket.c:1131-1251: the payload memcpy'd into
// MTU-sized frames, frag = offset >> 3 | MF) and, per frame, pico_ipv4_frame_push
// (modules/pico_ipv4.c:1039-1079: len, the shared id, frag, pico_ipv4_checksum);
// pico_ipv4_rebound_large (:1464-1510) applies the same split rule to a large ICMP reply.  The
// reference sends fragmented UDP with crc = 0 (modules/pico_udp.c:119-123: nothing sums the whole
// payload); here the pass that scatters the transport reads every byte once anyway, so the
// whole-datagram transport checksum comes with it.
//
// One workgroup per datagram; every check is made before the first store (a MALFORMED datagram
// writes nothing into its region):
//   1. the 20 template bytes (one lane each): the header's word sum without len / frag / crc and
//      the pseudo header's address part, once per datagram;
//   2. wave w takes the fragment pairs w, w + 4, ... (one wave: every pair): fragments 2j and
//      2j + 1.  Lanes 0..19 write each fragment's header -- the template with len, frag and the
//      checksum from the template's sum plus those two words (no re-read).  The two payloads move
//      and enter the transport sum through the 16-byte unit mover (unit_pair_move, pico_csum_dev.h:
//      the unit scheme and the read rule are stated there), one sum for the whole datagram -- the
//      pairing is the datagram's because per is even; the readable block ends with the datagram;
//   3. the sum is reduced over the workgroup (DPP, then LDS); thread 0 takes the crc field's own
//      word out of it (the field reads as zero), adds the pseudo header and -- F_WRITE -- stores
//      the result into the fragment that holds the field, behind the barrier that orders it after
//      the scatter's store of the same bytes.
#include "pico_csum_dev.h"

namespace {

struct FragTxArgs {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* dgram;
    uint32_t n_dgram;
    uint32_t mtu;
    const uint32_t* grp;                // 2 per datagram: first slot, slots reserved
    uint32_t n_frag;
    uint32_t stride;
    uint8_t* out;
    uint64_t out_len;
    const pico_csum_desc_dev* odesc;    // per datagram: output region (off, capacity)
    pico_csum_desc_dev* o_frag;
    uint32_t* o_count;
    uint16_t* o_l4;
    uint8_t* verdict;
    uint32_t flags;
};

// FTX_WAVES waves per datagram, FTX_U 64-unit rows per step.  Launch shapes (measured:
// profiles/fragtx/): four waves and three rows (two 1480-byte payloads; 94 VGPRs),
// or -- large batches of short datagrams, SHORT_GROUPS_MIN / SHORT_SLOTS_AVG in pico_csum_dev.h --
// one wave and one row (64 VGPRs, 8 waves a SIMD).
template <uint32_t FTX_WAVES, uint32_t FTX_U>
__global__ __launch_bounds__(64 * FTX_WAVES) void fragment_kernel(FragTxArgs p) {
    __shared__ uint32_t s_acc[FTX_WAVES];
    const uint32_t g = blockIdx.x;
    if (g >= p.n_dgram) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const pico_csum_desc_dev d = p.dgram[g], od = p.odesc[g];
    const uint32_t first = p.grp[2 * g], reserved = p.grp[2 * g + 1];
    const uint32_t per = (p.mtu - 20u) & ~7u;                       // mtu >= 28: per >= 8

    // ---- checks (workgroup-uniform): nothing is stored for a datagram that fails one
    const bool slots_ok = slots_in(first, reserved, p.n_frag);
    bool bad = span_out(d, p.base_len) || d.len < 20u || d.len > 65535u || !slots_ok;
    const uint32_t tl = bad ? 0u : d.len - 20u;
    const bool whole = d.len <= p.mtu;                              // pico_ipv4.c:1059: frag = DF, one frame
    const SlotPlan sp = slot_plan(tl, per, p.stride, 20u, whole || tl == 0u);
    const uint32_t count = sp.count, last_pl = sp.last_pl;
    bad = bad || reserved < count || span_out(od, p.out_len) || sp.need > od.len;
    const uint8_t* h = p.base + d.off;
    if (!bad) bad = ((uint32_t)h[0] & 0x0Fu) != 5u;

    if (p.o_frag && slots_ok)
        write_slots(p.o_frag + first, reserved, bad ? 0u : count, od.off, p.stride, 20u, per, last_pl, tid, 64u * FTX_WAVES);
    if (bad) {
        if (tid == 0) {
            if (p.o_count) p.o_count[g] = 0u;
            if (p.o_l4) p.o_l4[g] = 0;
            if (p.verdict) p.verdict[g] = (uint8_t)V_MALFORMED;
        }
        return;
    }

    // ---- 1. the template: word sums of the header without len / frag / crc, and of src / dst
    const uint32_t hb = lane < 20u ? (uint32_t)h[lane] : 0u;
    const uint32_t hw = lane & 1u ? hb << 8 : hb;                   // the byte's place in its LE word
    const bool tmpl = lane < 20u && !(lane == 2u || lane == 3u || lane == 6u || lane == 7u || lane == 10u || lane == 11u);
    const uint32_t hsum = wave_total(tmpl ? hw : 0u);
    const uint32_t asum = wave_total(lane >= 12u && lane < 20u ? hw : 0u);
    const uint32_t proto = (uint32_t)__builtin_amdgcn_readlane((int)hb, 9);

    // ---- 2. scatter + sum
    const uint64_t S = reinterpret_cast<uint64_t>(h) + 20u;                         // the transport
    const uint64_t a1 = (reinterpret_cast<uint64_t>(h) + d.len + 15u) & ~(uint64_t)15;   // end of its last 16-byte block
    const uint64_t D = reinterpret_cast<uint64_t>(p.out) + od.off;                   // fragment 0's header
    uint32_t acc = 0;
    const uint32_t npair = (count + 1u) >> 1;
    for (uint32_t j = wv; j < npair; j += FTX_WAVES) {
        const uint32_t kA = 2u * j, kB = kA + 1u;
        const bool hasB = kB < count;
        const uint32_t plA = kA + 1u < count ? per : last_pl, plB = hasB ? (kB + 1u < count ? per : last_pl) : 0u;
        const uint64_t dA = D + (uint64_t)kA * p.stride, dB = D + (uint64_t)kB * p.stride;
        // the headers: the template's bytes with len, frag (offset >> 3 | MF; DF on a datagram sent
        // whole) and pico_ipv4_checksum
        if (lane < 20u) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (b == 1 && !hasB) break;
                const uint32_t k = b ? kB : kA, len = 20u + (b ? plB : plA);
                const uint32_t frag = whole ? 0x4000u : (((k * per) >> 3) | (k + 1u < count ? 0x2000u : 0u));
                const uint32_t crc = finalize(hsum + bswap16(len) + bswap16(frag));
                uint32_t v = hb;
                v = lane == 2u ? len >> 8 : (lane == 3u ? len & 0xFFu : v);
                v = lane == 6u ? frag >> 8 : (lane == 7u ? frag & 0xFFu : v);
                v = lane == 10u ? crc >> 8 : (lane == 11u ? crc & 0xFFu : v);
                reinterpret_cast<uint8_t*>(b ? dB : dA)[lane] = (uint8_t)v;
            }
        }

        const uint64_t sA = S + (uint64_t)kA * per, sB = S + (uint64_t)kB * per;
        // (cached whole-unit stores: non-temporal measured slower here)
        unit_pair_move<FTX_U, false, false>(sA, sB, dA + 20u, dB + 20u, a1, a1, plA, plB, hasB, lane, acc, acc);
    }
    acc = wave_total(acc);
    if (lane == 0) s_acc[wv] = acc;
    __syncthreads();        // (also orders the F_WRITE store below after the scatter's stores)

    // ---- 3. the transport checksum of the whole datagram, its crc field read as zero
    if (tid == 0) {
        uint32_t l4 = 0;
        const uint32_t crc_at = proto == 6u ? 16u : (proto == 17u ? 6u : (proto == 1u ? 2u : NONE));
        if (crc_at != NONE) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t k = 0; k < FTX_WAVES; ++k) s += s_acc[k];
            const bool field = crc_at + 2u <= tl;                   // the field lies inside the transport
            const uint8_t* t = h + 20u;
            if (field) s -= (uint32_t)t[crc_at] | ((uint32_t)t[crc_at + 1u] << 8);
            if (proto != 1u) s += asum + (proto << 8) + bswap16(tl);     // struct pico_ipv4_pseudo_hdr as LE words
            l4 = finalize(s);
            if (field && (p.flags & 1u)) {                          // PICO_CSUM_F_WRITE
                const uint32_t kf = whole ? 0u : crc_at / per;      // the fragment that holds the field
                store_crc(p.out + od.off + (uint64_t)kf * p.stride + 20u + (crc_at - kf * per), l4);
            }
        }
        if (p.o_count) p.o_count[g] = count;
        if (p.o_l4) p.o_l4[g] = (uint16_t)l4;
        if (p.verdict) p.verdict[g] = (uint8_t)V_ACCEPT;
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_fragment(const void* base, uint64_t base_len, const void* dgram, uint32_t n_dgram, uint32_t mtu,
                              const uint32_t* groups, uint32_t n_frag, void* out, uint64_t out_len, const void* out_desc,
                              uint32_t stride, void* o_frag, uint32_t* o_count, uint16_t* o_l4, uint8_t* verdict,
                              uint32_t flags, void* stream) {
    if (n_dgram == 0) return (int)hipSuccess;
    FragTxArgs a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(dgram), n_dgram, mtu,
                 groups, n_frag, stride, static_cast<uint8_t*>(out), out_len,
                 static_cast<const pico_csum_desc_dev*>(out_desc), static_cast<pico_csum_desc_dev*>(o_frag), o_count,
                 o_l4, verdict, flags};
    if (short_groups(n_dgram, n_frag))
        hipLaunchKernelGGL((fragment_kernel<1u, 1u>), dim3(n_dgram), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((fragment_kernel<4u, 3u>), dim3(n_dgram), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
