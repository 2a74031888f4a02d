// viterbi.hip -- the decoder's Viterbi27 on the GPU (decoder/src/newdecoder.cpp:272-300): every valid frame of a call
// is one window of 64 carry symbols + 16384 frame symbols, decoded by maximum likelihood over its 8224 bits.
//
// Contract (DESIGN.md "Frame decoder"): the register takes new bits at its low end, the state is the newest 6 bits,
// the expected symbol of coded bit c is 1 - 2c, branch metric s[2t] ea + s[2t+1] ec (maximised), all 64 start metrics
// 0, a tie keeps the predecessor ns >> 1, the end state is the first state with the largest metric.  int32 metrics
// never overflow (|metric| <= 256 * 8224 < 2^22), so the decisions are exact and equal to the test side's.
//
// Layout: one wave per window, one state per lane.  Successor ns comes from ns >> 1 (bit 6 = 0) or (ns >> 1) | 32
// (bit 6 = 1); the second register differs from the first in bit 6 only, which both generators tap, so its branch
// metric is the first one negated.  Two ds_bpermute per step fetch the predecessors' metrics, a ballot records the
// 64 decisions, and lane i of a chunk keeps step i's word, so that a chunk of 64 steps leaves with one coalesced
// 512-byte store.  The symbols of a chunk come in with one load per lane and are broadcast by readlane.
//
// Traceback: the chunk's 64 decision words come back with one coalesced load and the wave walks them with readlane
// (the state is wave-uniform).  Lane i keeps the register of step i, so after the chunk every lane re-encodes its own
// step for viterbi_errors, and a ballot of the decoded bits is the chunk's 64 bits in time order: NRZ-M (HRIT), bit
// order and the 8-byte store are then a handful of scalar operations.  Chunk 0 holds steps 0..31 (the carry's 32
// bits), chunk c >= 1 steps 64c - 32 .. 64c + 31, which are CADU bytes 8(c-1) .. 8(c-1)+7.
#include "kernels.h"

namespace xrit {

constexpr int VIT_FRAME = FRAME_SYMBOLS;
constexpr int VIT_CARRY = 64;
constexpr int VIT_STEPS = (VIT_FRAME + VIT_CARRY) / 2;       // 8224
constexpr int VIT_CHUNKS = 129;                              // 32 + 128 * 64 steps
constexpr size_t VIT_SLOT_WORDS = (size_t)VIT_CHUNKS * 64;   // decision words per resident window
static_assert(32 + (VIT_CHUNKS - 1) * 64 == VIT_STEPS, "chunk 0 holds 32 steps, the others 64");

__device__ __forceinline__ int vit_t0(int c) { return c == 0 ? 0 : 64 * c - 32; }
__device__ __forceinline__ int vit_len(int c) { return c == 0 ? 32 : 64; }

// soft symbol i of frame f's window: the carry (the most recent earlier valid frame of the call, or the handle's
// carry) for i < 64, the frame after that
__device__ __forceinline__ int vit_symbol(const int8_t *__restrict__ frames, const int8_t *__restrict__ carry_src, size_t f,
                                          int i)
{
    return i < VIT_CARRY ? (int)carry_src[i] : (int)frames[f * VIT_FRAME + (size_t)(i - VIT_CARRY)];
}

// the step-t symbol pair of lane-step t, packed s0 | s1 << 8 (bytes as they are)
__device__ __forceinline__ int vit_pair(const int8_t *__restrict__ frames, const int8_t *__restrict__ carry_src, size_t f,
                                        int t)
{
    const int s0 = vit_symbol(frames, carry_src, f, 2 * t), s1 = vit_symbol(frames, carry_src, f, 2 * t + 1);
    return (s0 & 0xFF) | ((s1 & 0xFF) << 8);
}

__device__ __forceinline__ int vit_parity(int v) { return __popc((unsigned)v) & 1; }

// prev[f] = the most recent valid frame before f in this call (-1: none, the handle's carry), *last = the call's last
// valid frame (-1: none).  One workgroup: a segment of frames per thread, then a max-scan across the segments.
__global__ void __launch_bounds__(1024) vit_scan_kernel(const unsigned char *__restrict__ valid, unsigned nf, int *__restrict__ prev,
                                                        int *__restrict__ last)
{
    __shared__ int seg_last[1024];
    const unsigned tid = threadIdx.x, per = (nf + 1023) / 1024;
    const unsigned a = tid * per, b = min(nf, a + per);
    int l = -1;
    for (unsigned f = a; f < b; ++f)
        if (valid[f]) l = (int)f;
    seg_last[tid] = l;
    __syncthreads();
    for (unsigned off = 1; off < 1024; off <<= 1) {           // inclusive max-scan (Hillis-Steele)
        const int v = tid >= off ? seg_last[tid - off] : -1;
        __syncthreads();
        seg_last[tid] = max(seg_last[tid], v);
        __syncthreads();
    }
    int run = tid ? seg_last[tid - 1] : -1;
    for (unsigned f = a; f < b; ++f) {
        prev[f] = run;
        if (valid[f]) run = (int)f;
    }
    if (tid == 1023) *last = seg_last[1023];
}

__global__ void __launch_bounds__(64) vit_decode_kernel(const int8_t *__restrict__ frames, const unsigned char *__restrict__ valid,
                                                        const int *__restrict__ prev, const int8_t *__restrict__ carry,
                                                        unsigned nf, int hrit, unsigned long long *__restrict__ dec_all,
                                                        unsigned char *__restrict__ cadu, unsigned *__restrict__ verr)
{
    const int lane = threadIdx.x;
    unsigned long long *__restrict__ dec = dec_all + (size_t)blockIdx.x * VIT_SLOT_WORDS;
    // this lane's state ns = lane: predecessors j = ns >> 1 and j | 32, branch metric of the bit-6 = 0 register
    const int ea = 1 - 2 * vit_parity(lane & 0x4F), ec = 1 - 2 * vit_parity(lane & 0x6D);
    const int src0 = (lane >> 1) * 4, src1 = ((lane >> 1) | 32) * 4;
    for (unsigned f = blockIdx.x; f < nf; f += gridDim.x) {
        unsigned char *out = cadu + (size_t)f * 1024;
        if (!valid[f]) {
            reinterpret_cast<uint4 *>(out)[lane] = make_uint4(0, 0, 0, 0);
            if (lane == 0) verr[f] = 0;
            continue;
        }
        const int p = prev[f];
        const int8_t *carry_src = p >= 0 ? frames + (size_t)p * VIT_FRAME + (VIT_FRAME - VIT_CARRY) : carry;
        // ---- add-compare-select ----
        int pm = 0;
        int sym = vit_pair(frames, carry_src, f, lane);
        for (int c = 0; c < VIT_CHUNKS; ++c) {
            const int t0 = vit_t0(c), len = vit_len(c);
            const int cn = c + 1 < VIT_CHUNKS ? c + 1 : c;
            const int sym_next = vit_pair(frames, carry_src, f, vit_t0(cn) + lane);     // lanes past 8223 read the
            unsigned long long mine = 0;                                              // last chunk's tail: unused
            for (int i = 0; i < len; ++i) {
                const int v = __builtin_amdgcn_readlane(sym, i);
                const int s0 = (int)(int8_t)(v & 0xFF), s1 = (int)(int8_t)((v >> 8) & 0xFF);
                const int bm = s0 * ea + s1 * ec;
                const int c0 = __builtin_amdgcn_ds_bpermute(src0, pm) + bm;
                const int c1 = __builtin_amdgcn_ds_bpermute(src1, pm) - bm;
                const bool take1 = c1 > c0;
                pm = take1 ? c1 : c0;
                const unsigned long long d = __ballot(take1);
                mine = lane == i ? d : mine;
            }
            if (lane < len) dec[t0 + lane] = mine;
            sym = sym_next;
        }
        // ---- end state: the first state with the largest metric ----
        // (this loop and the error sum below stay written out: as a wave maximum and wave_ops.h's wave_sum the kernel came out
        // with other registers and block order, and the decode call measured 0.05 ms in 47.5 ms slower)
        unsigned key = ((unsigned)(pm + (1 << 23)) << 6) | (unsigned)(63 - lane);
        for (int off = 32; off > 0; off >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, off, 64));
        int st = 63 - (int)(key & 63u);
        __threadfence_block();                                  // the decision words this wave stored, read back below
        // ---- traceback, re-encoding and output, last chunk first ----
        unsigned err = 0;
        unsigned long long w = dec[vit_t0(VIT_CHUNKS - 1) + lane];
        for (int c = VIT_CHUNKS - 1; c >= 0; --c) {
            const int t0 = vit_t0(c), len = vit_len(c);
            const unsigned long long w_next = c > 0 ? dec[vit_t0(c - 1) + (lane < vit_len(c - 1) ? lane : 0)] : 0ull;
            const unsigned wlo = (unsigned)w, whi = (unsigned)(w >> 32);
            int reg = 0;
            for (int i = len - 1; i >= 0; --i) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)wlo, i);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)whi, i);
                const int d = (int)(((st < 32 ? lo >> st : hi >> (st - 32))) & 1u);
                const int r = st | (d << 6);
                reg = lane == i ? r : reg;
                st = (st >> 1) | (d << 5);
            }
            const bool in = lane < len;
            if (in) {
                const int v = vit_pair(frames, carry_src, f, t0 + lane);
                const int s0 = (int)(int8_t)(v & 0xFF), s1 = (int)(int8_t)((v >> 8) & 0xFF);
                const int e0 = 1 - 2 * vit_parity(reg & 0x4F), e1 = 1 - 2 * vit_parity(reg & 0x6D);
                err += (s0 * e0 < 0 ? 1u : 0u) + (s1 * e1 < 0 ? 1u : 0u);
            }
            unsigned long long bits = __ballot(in && (reg & 1));
            if (c > 0) {
                if (hrit) bits ^= (bits << 1) | (unsigned long long)(st & 1);       // st: the state after step t0 - 1
                // bit l is time t0 + l; bytes are sent MSB first
                const unsigned long long be = __builtin_bswap64(__builtin_bitreverse64(bits));
                if (lane == 0) *reinterpret_cast<unsigned long long *>(out + 8 * (c - 1)) = be;
            }
            w = w_next;
        }
        for (int off = 32; off > 0; off >>= 1) err += (unsigned)__shfl_xor((int)err, off, 64);
        if (lane == 0) verr[f] = err;
    }
}

// the handle's carry: the last 64 symbols of the call's last valid frame (left as it is when there is none)
__global__ void __launch_bounds__(64) vit_carry_kernel(const int8_t *__restrict__ frames, const int *__restrict__ last,
                                                       int8_t *__restrict__ carry)
{
    const int l = *last;
    if (l >= 0) carry[threadIdx.x] = frames[(size_t)l * VIT_FRAME + (VIT_FRAME - VIT_CARRY) + threadIdx.x];
}

size_t viterbi_slot_bytes() { return VIT_SLOT_WORDS * sizeof(unsigned long long); }

int launch_viterbi(const int8_t *frames, const unsigned char *valid, size_t nf, int hrit, int8_t *carry, int *prev, int *last,
                   unsigned long long *dec, unsigned slots, unsigned char *cadu, unsigned *verr, hipStream_t s)
{
    if (nf == 0) return XRIT_OK;
    hipLaunchKernelGGL(vit_scan_kernel, dim3(1), dim3(1024), 0, s, valid, (unsigned)nf, prev, last);
    XR_HIP(hipGetLastError());
    const unsigned grid = nf < slots ? (unsigned)nf : slots;
    hipLaunchKernelGGL(vit_decode_kernel, dim3(grid), dim3(64), 0, s, frames, valid, prev, carry, (unsigned)nf, hrit, dec, cadu,
                       verr);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(vit_carry_kernel, dim3(1), dim3(64), 0, s, frames, last, carry);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
