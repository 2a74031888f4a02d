// rs.hip -- DeRandomizer + 4 x ReedSolomon::decode_ccsds + the header fields of newdecoder.cpp:302-348, one wave per
// frame.  The wave XORs the CADU's 1020 bytes behind the ASM with the PN sequence (:304-307), maps the bytes from the
// dual basis into LDS (de-interleaved: codeword k holds bytes j = 4i + k, :313-318), and computes the 4 x 32
// syndromes two per lane by Horner with log / antilog tables in LDS.  A codeword with all syndromes zero -- every
// codeword of a clean frame -- is done.  Otherwise one lane per codeword runs Berlekamp-Massey, the Chien search and
// Forney (rs_core.h) and corrects the bytes in place; an uncorrectable codeword (-1) passes through byte for byte.
// The frame is ok unless all four codewords are -1 (:321).
#include "kernels.h"
#include "rs_core.h"

namespace xrit {

__constant__ RsTables c_rs = rs_make_tables();

__global__ void __launch_bounds__(64) rs_decode_kernel(const unsigned char *__restrict__ cadu, const unsigned char *__restrict__ valid,
                                                       const unsigned *__restrict__ verr, unsigned nf,
                                                       unsigned char *__restrict__ block, xrit_frame_info *__restrict__ info)
{
    __shared__ uint8_t ex[512], lg[256], to_dual[256], to_conv[256];
    __shared__ uint8_t r[1024];              // the derandomised block (wire basis), corrected in place
    __shared__ uint8_t cw[4][256];           // the four codewords in the conventional basis
    __shared__ uint8_t S[4][RS_NROOTS];
    __shared__ int rs_err[4];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    unsigned char *out = block + f * 1020;
    if (!valid[f]) {
        for (int j = lane; j < 1020; j += 64) out[j] = 0;
        if (lane == 0) {
            xrit_frame_info z{};
            for (int k = 0; k < 4; ++k) z.rs_errors[k] = -1;
            info[f] = z;
        }
        return;
    }
    for (int i = lane; i < 512; i += 64) ex[i] = c_rs.exp[i];
    for (int i = lane; i < 256; i += 64) {
        lg[i] = c_rs.log[i];
        to_dual[i] = c_rs.to_dual[i];
        to_conv[i] = c_rs.to_conv[i];
    }
    __syncthreads();
    const unsigned char *in = cadu + f * 1024 + 4;
    for (int j = lane; j < 1020; j += 64) {
        const uint8_t x = in[j] ^ c_rs.pn[j % 255];
        r[j] = x;
        cw[j & 3][j >> 2] = to_conv[x];
    }
    __syncthreads();
    // syndromes i0 and i0 + 16 of codeword k
    const int k = lane >> 4, i0 = lane & 15;
    const unsigned la = (unsigned)((RS_PRIM * (RS_FCR + i0)) % RS_NN), lb = (unsigned)((RS_PRIM * (RS_FCR + i0 + 16)) % RS_NN);
    unsigned sa = 0, sb = 0;
    for (int j = 0; j < RS_NN; ++j) {
        const unsigned c = cw[k][j];
        sa = (sa ? ex[lg[sa] + la] : 0u) ^ c;
        sb = (sb ? ex[lg[sb] + lb] : 0u) ^ c;
    }
    S[k][i0] = (uint8_t)sa;
    S[k][i0 + 16] = (uint8_t)sb;
    const unsigned long long bad = __ballot((sa | sb) != 0);
    __syncthreads();
    if (i0 == 0) {
        int n = 0;
        if ((bad >> (16 * k)) & 0xFFFFull) {
            int where[RS_T];
            uint8_t mag[RS_T];
            n = rs_solve(S[k], ex, lg, where, mag);
            for (int e = 0; e < n; ++e) {
                const int j = 4 * where[e] + k;
                r[j] = to_dual[to_conv[r[j]] ^ mag[e]];
            }
        }
        rs_err[k] = n;
    }
    __syncthreads();
    for (int j = lane; j < 1020; j += 64) out[j] = r[j];
    if (lane == 0) {
        xrit_frame_info o;
        o.valid = 1;
        o.ok = (rs_err[0] == -1 && rs_err[1] == -1 && rs_err[2] == -1 && rs_err[3] == -1) ? 0u : 1u;
        o.viterbi_errors = verr[f];
        for (int q = 0; q < 4; ++q) o.rs_errors[q] = rs_err[q];
        o.scid = ((r[0] & 0x3Fu) << 2) | ((r[1] & 0xC0u) >> 6);
        o.vcid = r[1] & 0x3Fu;
        o.counter = ((unsigned)r[2] << 16) | ((unsigned)r[3] << 8) | r[4];
        info[f] = o;
    }
}

int launch_rs(const unsigned char *cadu, const unsigned char *valid, const unsigned *verr, size_t nf, unsigned char *block,
              xrit_frame_info *info, hipStream_t s)
{
    if (nf == 0) return XRIT_OK;
    hipLaunchKernelGGL(rs_decode_kernel, dim3((unsigned)nf), dim3(64), 0, s, cadu, valid, verr, (unsigned)nf, block, info);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
