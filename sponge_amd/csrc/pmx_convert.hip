// squeeze_bytes / squeeze_bits of a batch of device-resident sponges (src/poseidon/mod.rs:256-286): the native squeeze of the width's
// engine into a scratch block, then one of the two kernels below, which turn the squeezed ABI residues [n][E][4] into the canonical
// integers' low bytes / bits, packed [n][len].  The kernels read ABI residues, so one instantiation serves every width, exponent and
// engine; this translation unit is compiled once and pmx_device.hip knows nothing of it.
//
// Shape of a kernel (cdna_hip_programming "Global memory coalescing"): a lane reads its element as two 16-byte loads and converts it
// (abi_to_canonical: 81 multiplies).  Its output record is 28 .. 31 bytes (bits: up to 254 bytes) at an arbitrary byte address, but
// the rows are packed, so the records of the consecutive elements of one workgroup form ONE contiguous byte span (pmx_squeeze_cut.hpp).
// The span is assembled in LDS at the address it has in global memory modulo 16 and streamed out as whole 16-byte stores over its
// aligned interior; only the two ragged ends of a workgroup's span (below 16 bytes each) take byte stores.  Nothing outside
// [out, out + n * len) is written, and no byte of it twice.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmx_launch.hpp"
#include "pmx_squeeze_cut.hpp"

namespace pmx {

constexpr uint32_t kCutThreads = 256;
constexpr uint32_t kByteElems = 256;   // elements per workgroup: one per lane
constexpr uint32_t kBitElems = 64;     // bits expand 8 x: one element per FOUR lanes, 64 bits each
constexpr uint32_t kMaxUnitBytes = 31, kMaxUnitBits = 254;   // p < 2^255
constexpr uint32_t kByteStage = (kByteElems * kMaxUnitBytes + 15 + 15) / 16;   // uint4: the span and its offset inside the first 16 bytes
constexpr uint32_t kBitStage = (kBitElems * kMaxUnitBits + 15 + 15) / 16;

// A record of `len` bytes - the little-endian bytes of K words of type W, word(j) for a compile-time j - to stage[q, q + len): the words
// are shifted to the alignment of q, words that lie inside the record are stored whole, the (at most two) that straddle an end byte by
// byte.  Lanes whose records touch never share a whole word.
template <class W, int K, class Word>
__device__ __forceinline__ void lds_deposit(uint8_t *stage, uint32_t q, uint32_t len, Word &&word) {
    constexpr uint32_t S = sizeof(W);
    const uint32_t sh = (q & (S - 1)) * 8, a0 = q & ~(S - 1), end = q + len;
    W prev = 0;
    static_for<0, K + 1>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        W cur = 0;
        if constexpr (j < K) cur = word(jj);
        const W v = sh ? (W)((cur << sh) | (prev >> (S * 8 - sh))) : cur;
        prev = cur;
        const uint32_t a = a0 + S * j;
        if (a >= q && a + S <= end) {
            *reinterpret_cast<W *>(stage + a) = v;
        } else if (a < end) {
#pragma unroll
            for (uint32_t b = 0; b < S; ++b)
                if (a + b >= q && a + b < end) stage[a + b] = (uint8_t)(v >> (8 * b));
        }
    });
}

// stage[a - base] -> global a for a in [lo, hi): 16-byte stores over the aligned interior, byte stores at the two ends
__device__ __forceinline__ void stream_span(const uint8_t *stage, uintptr_t base, uintptr_t lo, uintptr_t hi) {
    const uint32_t tid = threadIdx.x;
    uintptr_t in_lo = (lo + 15) & ~(uintptr_t)15;
    if (in_lo > hi) in_lo = hi;
    uintptr_t in_hi = hi & ~(uintptr_t)15;
    if (in_hi < in_lo) in_hi = in_lo;
    for (uintptr_t a = in_lo + 16 * (uintptr_t)tid; a < in_hi; a += 16 * (uintptr_t)kCutThreads)
        *reinterpret_cast<uint4 *>(a) = *reinterpret_cast<const uint4 *>(stage + (a - base));
    if (tid < in_lo - lo) *reinterpret_cast<uint8_t *>(lo + tid) = stage[lo + tid - base];
    if (tid >= 64 && tid - 64 < hi - in_hi) *reinterpret_cast<uint8_t *>(in_hi + (tid - 64)) = stage[in_hi + (tid - 64) - base];
}

// Element g = r * elems + e of the batch, for the `per` consecutive elements of a workgroup: its row and index, its position in the
// staged span.  One 64-bit division per workgroup (wave-uniform), 32-bit ones per lane.
struct CutSpan {
    uint64_t r0;
    uint32_t e0, cnt;
    uintptr_t lo, hi, base;
    __device__ __forceinline__ CutSpan(const uint8_t *out, uint64_t total, uint32_t elems, uint64_t len, uint32_t unit, uint32_t per) {
        const uint64_t g0 = (uint64_t)blockIdx.x * per;
        cnt = total - g0 < per ? (uint32_t)(total - g0) : per;
        r0 = g0 / elems;
        e0 = (uint32_t)(g0 - r0 * elems);
        lo = (uintptr_t)out + cut_offset(r0, e0, len, unit);
        hi = (uintptr_t)out + cut_offset(r0 + (e0 + cnt) / elems, (e0 + cnt) % elems, len, unit);
        base = lo & ~(uintptr_t)15;
    }
};

__global__ void __launch_bounds__(kCutThreads) squeeze_bytes_kernel(const uint32_t *__restrict__ in, uint8_t *__restrict__ out, const FieldRt f,
                                                                   uint64_t total, uint32_t elems, uint64_t len, uint32_t unit) {
    __shared__ uint4 stage4[kByteStage];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    const CutSpan sp(out, total, elems, len, unit, kByteElems);
    const uint32_t tid = threadIdx.x;
    if (tid < sp.cnt) {
        const uint64_t g = (uint64_t)blockIdx.x * kByteElems + tid;
        const uint32_t ee = sp.e0 + tid, e = ee % elems;
        const Abi x = abi_to_canonical(abi_load(in + g * 8), f);
        const uint32_t q = (uint32_t)((uintptr_t)out + cut_offset(sp.r0 + ee / elems, e, len, unit) - sp.base);
        lds_deposit<uint32_t, 8>(stage, q, cut_count(e, len, unit), [&](auto j) { return x.w[decltype(j)::value]; });
    }
    __syncthreads();
    stream_span(stage, sp.base, sp.lo, sp.hi);
}

// four bits -> four bytes holding 0 or 1, lowest bit first (to_bits_le): the shifted copies of the nibble do not overlap
__device__ __forceinline__ uint32_t spread4(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

__global__ void __launch_bounds__(kCutThreads) squeeze_bits_kernel(const uint32_t *__restrict__ in, uint8_t *__restrict__ out, const FieldRt f,
                                                                  uint64_t total, uint32_t elems, uint64_t len, uint32_t unit) {
    __shared__ uint4 canon4[kBitElems * 2];   // the canonical integers of the workgroup's elements, 8 words each
    __shared__ uint4 stage4[kBitStage];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    uint32_t *canon = reinterpret_cast<uint32_t *>(canon4);
    const CutSpan sp(out, total, elems, len, unit, kBitElems);
    const uint32_t tid = threadIdx.x;
    // the first wave converts, the other three wait at the barrier; other workgroups of the CU (up to 8 fit its LDS) fill the SIMDs
    // meanwhile.  Whether converting in all four waves would pay was not measured: the call is bound by the squeeze.
    if (tid < sp.cnt) {
        const uint64_t g = (uint64_t)blockIdx.x * kBitElems + tid;
        abi_store(canon + tid * 8, abi_to_canonical(abi_load(in + g * 8), f));
    }
    __syncthreads();
    const uint32_t el = tid >> 2, part = tid & 3;   // bits [64 part, 64 part + 64) of element el
    if (el < sp.cnt) {
        const uint32_t ee = sp.e0 + el, e = ee % elems;
        const uint32_t count = cut_count(e, len, unit);
        const uint32_t mine = count > 64 * part ? (count - 64 * part < 64 ? count - 64 * part : 64) : 0;
        const uint32_t w0 = canon[el * 8 + 2 * part], w1 = canon[el * 8 + 2 * part + 1];
        const uint32_t q = (uint32_t)((uintptr_t)out + cut_offset(sp.r0 + ee / elems, e, len, unit) - sp.base) + 64 * part;
        // eight bits become one 64-bit word of eight 0 / 1 bytes
        lds_deposit<uint64_t, 8>(stage, q, mine, [&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t byte = ((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xffu;
            return (uint64_t)spread4(byte & 15u) | (uint64_t)spread4(byte >> 4) << 32;
        });
    }
    __syncthreads();
    stream_span(stage, sp.base, sp.lo, sp.hi);
}

// The composition (as launch_hash_varlen composes): a block of the pass pool, the engine's squeeze of `elems` native elements into it,
// the conversion from it into `out`, `done` behind the last conversion launch.  A call whose n * elems * 32 bytes exceed kCutScratchBytes
// runs slice by slice over SPONGES through one block (a slice is at least one sponge: scratch <= max(kCutScratchBytes, elems * 32)).
hipError_t launch_squeeze_cut(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, uint8_t *out, size_t len,
                              bool bits, size_t n, hipStream_t st, const PassScratch &scratch) {
    const uint32_t unit = cut_unit(c.field, bits);
    const size_t elems = cut_elems(len, unit);
    if (elems == 0) return launch_squeeze(c, t, states, tag, index, nullptr, 0, n, st, scratch);   // still permutes an Absorbing sponge
    size_t per = kCutScratchBytes / (elems * 32);
    if (per == 0) per = 1;
    if (per > n) per = n;
    PassLease lease(scratch, st);   // given back behind the last conversion launch
    hipError_t e = lease.take(per * elems * 32);
    if (e != hipSuccess) return e;
    uint32_t *block = lease.block;
    FieldRt f = c.field;
    f.io = c.consts + c.io_offset;
    for (size_t first = 0; first < n && e == hipSuccess; first += per) {
        const size_t cnt = n - first < per ? n - first : per;
        e = launch_squeeze(c, t, states + first * t * 4, tag + first, index + first, reinterpret_cast<uint64_t *>(block), elems, cnt, st, scratch);
        if (e != hipSuccess) break;
        const uint64_t total = (uint64_t)cnt * elems;
        uint8_t *dst = out + first * len;
        const uint32_t group = bits ? kBitElems : kByteElems;   // elements per workgroup
        hipLaunchKernelGGL(bits ? squeeze_bits_kernel : squeeze_bytes_kernel, dim3((unsigned)((total + group - 1) / group)), dim3(kCutThreads), 0, st,
                           block, dst, f, total, (uint32_t)elems, (uint64_t)len, unit);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace pmx
