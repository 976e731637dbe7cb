// pico_csum_k_fragtx6.hip -- IPv6 TX fragmentation scatter fused with the transport checksum of the
// whole datagram, and its launcher: the inverse of the IPv6 reassembly gather (pico_csum_k_frag.hip)
// and the IPv6 sibling of pico_csum_k_fragtx.hip.  Helpers and the arithmetic contract:
// pico_csum_dev.h.  The contract: include/pico_csum.h, pico_ipv6_fragment_batch_dev.
//
// Reference: none on the sending side -- pico_socket_xmit_fragments "Can't fragment IPv6" and cuts
// the datagram to one MTU (stack/pico_socket.c:1179-1185).  The split is RFC 8200 4.5's; what pins
// it is the reference's receiver, pico_ipv6_process_frag (modules/pico_fragments.c:432-498), which
// must put the fragments together again (tests/golden/make_ref_fragtx6.py).
//
// One workgroup per datagram; every check is made before the first store (a MALFORMED datagram
// writes nothing into its region):
//   1. the 40 template bytes (one lane each): the pseudo header's address part, the next header,
//      once per datagram.  An IPv6 header has no checksum of its own: a fragment's 48 header bytes
//      are the template's with the payload length, next header 44 and the fragment header (next
//      header, 0, offset | M, id) -- only the payload length and the offset word vary;
//   2. wave w takes the fragment pairs w, w + 4, ... (one wave: every pair): fragments 2j and
//      2j + 1.  Lanes 0..47 write each fragment's header (0..39 for a datagram sent whole).  The
//      two payloads move and enter the transport sum through the 16-byte unit mover
//      (unit_pair_move, pico_csum_dev.h), one sum for the whole datagram -- the pairing is the
//      datagram's because per is even; the readable block ends with the datagram;
//   3. the sum is reduced over the workgroup (DPP, then LDS); thread 0 takes the crc field's own
//      word out of it (the field reads as zero), adds struct pico_ipv6_pseudo_hdr and -- F_WRITE --
//      stores the result into the fragment that holds the field, behind the barrier that orders it
//      after the scatter's store of the same bytes.
#include "pico_csum_dev.h"

namespace {

struct FragTx6Args {
    const uint8_t* base;
    uint64_t base_len;
    const pico_csum_desc_dev* dgram;    // seed: the fragment identification, host order
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

// The next-header values of extension headers (pico_ipv6.h: hop-by-hop, routing, fragment, ESP,
// AUTH, destination options, mobility): an unfragmentable part is out of scope.
__device__ __forceinline__ bool is_exthdr(uint32_t nx) {
    return nx == 0u || nx == 43u || nx == 44u || nx == 50u || nx == 51u || nx == 60u || nx == 135u;
}

// FT6_WAVES waves per datagram, FT6_U 64-unit rows per step.  Launch shapes: K8's two, taken over
// as they stand: four waves and three rows (two 1448-byte payloads fill them as
// two 1480-byte ones do), or -- short_groups, pico_csum_dev.h -- one wave and one row.
template <uint32_t FT6_WAVES, uint32_t FT6_U>
__global__ __launch_bounds__(64 * FT6_WAVES) void fragment6_kernel(FragTx6Args p) {
    __shared__ uint32_t s_acc[FT6_WAVES];
    const uint32_t g = blockIdx.x;
    if (g >= p.n_dgram) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const pico_csum_desc_dev d = p.dgram[g], od = p.odesc[g];
    const uint32_t first = p.grp[2 * g], reserved = p.grp[2 * g + 1];
    const uint32_t per = (p.mtu - 48u) & ~7u;                       // mtu >= 56: per >= 8 (RFC 8200 4.5)

    // ---- checks (workgroup-uniform): nothing is stored for a datagram that fails one
    const bool slots_ok = slots_in(first, reserved, p.n_frag);
    bool bad = span_out(d, p.base_len) || d.len < 40u || d.len > 65535u || !slots_ok;
    const uint32_t tl = bad ? 0u : d.len - 40u;
    const bool whole = d.len <= p.mtu;                              // no fragment header: 40 header bytes
    const uint32_t HB = whole ? 40u : 48u;                          // (slot_plan takes the one that applies)
    const SlotPlan sp = slot_plan(tl, per, p.stride, HB, whole || tl == 0u);
    const uint32_t count = sp.count, last_pl = sp.last_pl;
    bad = bad || reserved < count || span_out(od, p.out_len) || sp.need > od.len;
    const uint8_t* h = p.base + d.off;
    if (!bad) bad = ((uint32_t)h[0] >> 4) != 6u || is_exthdr((uint32_t)h[6]);

    if (p.o_frag && slots_ok)
        write_slots(p.o_frag + first, reserved, bad ? 0u : count, od.off, p.stride, HB, per, last_pl, tid, 64u * FT6_WAVES);
    if (bad) {
        if (tid == 0) {
            if (p.o_count) p.o_count[g] = 0u;
            if (p.o_l4) p.o_l4[g] = 0;
            if (p.verdict) p.verdict[g] = (uint8_t)V_MALFORMED;
        }
        return;
    }

    // ---- 1. the template: its bytes, the word sum of src / dst, the next header
    const uint32_t hb = lane < 40u ? (uint32_t)h[lane] : 0u;
    const uint32_t hw = lane & 1u ? hb << 8 : hb;                   // the byte's place in its LE word
    const uint32_t asum = wave_total(lane >= 8u && lane < 40u ? hw : 0u);
    const uint32_t nx = (uint32_t)__builtin_amdgcn_readlane((int)hb, 6);

    // ---- 2. scatter + sum
    const uint64_t S = reinterpret_cast<uint64_t>(h) + 40u;                         // the transport
    const uint64_t a1 = (reinterpret_cast<uint64_t>(h) + d.len + 15u) & ~(uint64_t)15;   // end of its last 16-byte block
    const uint64_t D = reinterpret_cast<uint64_t>(p.out) + od.off;                   // fragment 0's header
    uint32_t acc = 0;
    const uint32_t npair = (count + 1u) >> 1;
    for (uint32_t j = wv; j < npair; j += FT6_WAVES) {
        const uint32_t kA = 2u * j, kB = kA + 1u;
        const bool hasB = kB < count;
        const uint32_t plA = kA + 1u < count ? per : last_pl, plB = hasB ? (kB + 1u < count ? per : last_pl) : 0u;
        const uint64_t dA = D + (uint64_t)kA * p.stride, dB = D + (uint64_t)kB * p.stride;
        // the headers: the template's bytes with the payload length and -- a fragment -- next header
        // 44 and the fragment header {the template's next header, 0, offset | M, id}
        if (lane < HB) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (b == 1 && !hasB) break;
                const uint32_t k = b ? kB : kA, plen = (whole ? 0u : 8u) + (b ? plB : plA);
                const uint32_t om = k * per | (k + 1u < count ? 1u : 0u);
                uint32_t v = hb;
                v = lane == 4u ? plen >> 8 : (lane == 5u ? plen & 0xFFu : v);
                v = lane == 6u && !whole ? 44u : v;
                v = lane == 40u ? nx : v;                           // (41: reserved, 0 = hb)
                v = lane == 42u ? om >> 8 : (lane == 43u ? om & 0xFFu : v);
                v = lane >= 44u ? (d.seed >> (8u * ((47u - lane) & 3u))) & 0xFFu : v;
                reinterpret_cast<uint8_t*>(b ? dB : dA)[lane] = (uint8_t)v;
            }
        }

        const uint64_t sA = S + (uint64_t)kA * per, sB = S + (uint64_t)kB * per;
        // (cached whole-unit stores, as K8: non-temporal measured slower there)
        unit_pair_move<FT6_U, false, false>(sA, sB, dA + HB, dB + HB, a1, a1, plA, plB, hasB, lane, acc, acc);
    }
    acc = wave_total(acc);
    if (lane == 0) s_acc[wv] = acc;
    __syncthreads();        // (also orders the F_WRITE store below after the scatter's stores)

    // ---- 3. the transport checksum of the whole datagram, its crc field read as zero: the TX rule
    // of pico_ipv6_checksum_batch_dev (ipv6_dispatch, pico_csum_k_sorted.hip) -- TCP / UDP / ICMPv6
    // with a transport of at least its header, the value stored as computed; 0 otherwise
    if (tid == 0) {
        uint32_t l4 = 0;
        const uint32_t crc_at = nx == 6u ? 16u : (nx == 17u ? 6u : (nx == 58u ? 2u : NONE));
        if (crc_at != NONE && tl >= (nx == 6u ? 20u : (nx == 17u ? 8u : 4u))) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t k = 0; k < FT6_WAVES; ++k) s += s_acc[k];
            const uint8_t* t = h + 40u;
            s -= (uint32_t)t[crc_at] | ((uint32_t)t[crc_at + 1u] << 8);
            s += asum + bswap16(tl) + (nx << 8);                    // struct pico_ipv6_pseudo_hdr as LE words (tl < 2^16)
            l4 = finalize(s);
            if (p.flags & 1u) {                                     // PICO_CSUM_F_WRITE
                const uint32_t kf = whole ? 0u : crc_at / per;      // the fragment that holds the field
                store_crc(p.out + od.off + (uint64_t)kf * p.stride + HB + (crc_at - kf * per), l4);
            }
        }
        if (p.o_count) p.o_count[g] = count;
        if (p.o_l4) p.o_l4[g] = (uint16_t)l4;
        if (p.verdict) p.verdict[g] = (uint8_t)V_ACCEPT;
    }
}

}  // namespace

extern "C" {

int pico_csum_launch_fragment6(const void* base, uint64_t base_len, const void* dgram, uint32_t n_dgram, uint32_t mtu,
                               const uint32_t* groups, uint32_t n_frag, void* out, uint64_t out_len, const void* out_desc,
                               uint32_t stride, void* o_frag, uint32_t* o_count, uint16_t* o_l4, uint8_t* verdict,
                               uint32_t flags, void* stream) {
    if (n_dgram == 0) return (int)hipSuccess;
    FragTx6Args a{static_cast<const uint8_t*>(base), base_len, static_cast<const pico_csum_desc_dev*>(dgram), n_dgram, mtu,
                  groups, n_frag, stride, static_cast<uint8_t*>(out), out_len,
                  static_cast<const pico_csum_desc_dev*>(out_desc), static_cast<pico_csum_desc_dev*>(o_frag), o_count,
                  o_l4, verdict, flags};
    if (short_groups(n_dgram, n_frag))
        hipLaunchKernelGGL((fragment6_kernel<1u, 1u>), dim3(n_dgram), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL((fragment6_kernel<4u, 3u>), dim3(n_dgram), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
