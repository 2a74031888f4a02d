// rice.cpp -- C ABI of the Rice decoder (include/xritdemod_amd.h, "File assembler and Rice decoder"): stateless, the
// kernels are in rice.hip.  The host-buffer call stages through grow-only device buffers that the calling thread keeps
// (one set per thread, for the device it last used, kept until the process ends): no allocation once warmed up.
#include "common.h"
#include "kernels.h"

#include <atomic>

using namespace xrit;

namespace {
std::atomic<int> g_form{XRIT_RICE_FORM_DEFAULT};
int kernel_form()
{
    const int f = g_form.load();
    return f == XRIT_RICE_FORM_LANE ? RICE_FORM_LANE : RICE_FORM_WAVE;      // the default is the wave form: DESIGN.md section 16
}
struct Staging {
    int device = -1;
    DevBuf in, desc, out, status;
    void release() { for (DevBuf *b : {&in, &desc, &out, &status}) b->release(); }
};
thread_local Staging t_staging;
}  // namespace

int xrit_rice_form(int form)
{
    if (form != XRIT_RICE_FORM_DEFAULT && form != XRIT_RICE_FORM_LANE && form != XRIT_RICE_FORM_WAVE) {
        set_error("rice: no such kernel form %d", form);
        return XRIT_E_ARG;
    }
    g_form.store(form);
    return XRIT_OK;
}

static int check_args(const void *bytes, size_t n_bytes, const void *desc, size_t stride, size_t n_lines, int n, int J, int S,
                      const void *out, const void *status)
{
    if (n < 1 || n > 16 || !(J == 8 || J == 16 || J == 32 || J == 64) || S < 1 || S > 65535) {
        set_error("rice: bits per sample 1 .. 16, block 8 / 16 / 32 / 64, samples 1 .. 65535 (got %d, %d, %d)", n, J, S);
        return XRIT_E_ARG;
    }
    if (stride < 16 || (stride & 7) || n_lines > MAX_ROWS_PER_CALL) {
        set_error("rice: the descriptor stride is a multiple of 8 from 16 on, at most 2^24 lines per call");
        return XRIT_E_ARG;
    }
    if ((n_bytes && !bytes) || (n_lines && (!desc || !out || !status)) || ((size_t)desc & 7) || (n > 8 && ((size_t)out & 1))) {
        set_error("rice: null or misaligned argument");
        return XRIT_E_ARG;
    }
    return XRIT_OK;
}

int xrit_rice_decode_device(const uint8_t *d_bytes, size_t n_bytes, const void *d_desc, size_t stride, size_t n_lines,
                            int bits_per_sample, int block, int samples, void *d_out, uint8_t *d_status, int device, void *stream)
{
    XR_TRY(check_args(d_bytes, n_bytes, d_desc, stride, n_lines, bits_per_sample, block, samples, d_out, d_status));
    XR_TRY(select_device(device));
    return launch_rice(d_bytes, n_bytes, d_desc, stride, n_lines, bits_per_sample, block, samples, d_out, d_status, kernel_form(),
                       (hipStream_t)stream);
}

int xrit_rice_decode(const uint8_t *bytes, size_t n_bytes, const void *desc, size_t stride, size_t n_lines, int bits_per_sample,
                     int block, int samples, void *out, uint8_t *status, int device)
{
    XR_TRY(check_args(bytes, n_bytes, desc, stride, n_lines, bits_per_sample, block, samples, out, status));
    XR_TRY(select_device(device));
    if (n_lines == 0) return XRIT_OK;
    const size_t out_bytes = n_lines * (size_t)samples * (bits_per_sample <= 8 ? 1 : 2);
    Staging &st = t_staging;
    if (st.device != device) {
        st.release();
        st.device = device;
    }
    XR_TRY(st.in.reserve(n_bytes + 8));
    XR_TRY(st.desc.reserve(n_lines * stride));
    XR_TRY(st.out.reserve(out_bytes));
    XR_TRY(st.status.reserve(n_lines));
    if (n_bytes) XR_HIP(hipMemcpy(st.in.p, bytes, n_bytes, hipMemcpyHostToDevice));
    XR_HIP(hipMemcpy(st.desc.p, desc, n_lines * stride, hipMemcpyHostToDevice));
    XR_TRY(launch_rice(st.in.as<unsigned char>(), n_bytes, st.desc.p, stride, n_lines, bits_per_sample, block, samples, st.out.p,
                       st.status.as<unsigned char>(), kernel_form(), nullptr));
    XR_HIP(hipMemcpy(out, st.out.p, out_bytes, hipMemcpyDeviceToHost));
    XR_HIP(hipMemcpy(status, st.status.p, n_lines, hipMemcpyDeviceToHost));
    return XRIT_OK;
}
