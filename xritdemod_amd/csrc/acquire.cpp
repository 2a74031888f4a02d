// acquire.cpp -- C ABI of the carrier acquisition stage (include/xritdemod_amd.h, "Carrier acquisition"): the handle owns
// the state (one xrit_acquire_state), the tables (twiddles and window, computed in double once) and grow-only scratch in
// device memory; the kernels are in acquire.hip, the plain host parts in acquire_host.h.
#include <cstddef>
#include <vector>

#include "acquire_host.h"
#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_acquire_params) == 24 && offsetof(xrit_acquire_params, min_ratio) == 16, "xrit_acquire_params layout");
static_assert(sizeof(xrit_acquire_estimate_record) == 64 && offsetof(xrit_acquire_estimate_record, ratio) == 16 &&
                  offsetof(xrit_acquire_estimate_record, inc) == 40 && offsetof(xrit_acquire_estimate_record, applied) == 48,
              "xrit_acquire_estimate_record layout (ACQUIRE_RECORD_DTYPE mirrors it)");
static_assert(sizeof(xrit_acquire_state) == 40, "xrit_acquire_state layout (ACQUIRE_STATE_DTYPE mirrors it)");

struct xrit_acquire : StageHandle {
    xrit_acquire_params par{};
    DevBuf state, tables, scratch;
    DevBuf h_in, h_out, h_record;                   // the host-buffer forms'
    xrit_acquire_state *st() const { return state.as<xrit_acquire_state>(); }
    const float2 *tw() const { return tables.as<float2>(); }
    const float *win() const { return reinterpret_cast<const float *>(tables.as<char>() + (size_t)ACQ_N * 8); }
    void close_all() { close({&state, &tables, &scratch, &h_in, &h_out, &h_record}); }
};

int xrit_acquire_create(xrit_acquire **out, const xrit_acquire_params *params, int device)
{
    if (!out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    xrit_acquire_params par;
    if (!params || !acquire_params_resolve(*params, par)) {
        set_error("acquire: sample_rate > 0, pre_sum 1 .. %u, segments %u .. %u, min_ratio > 0 (0 selects a default)", ACQ_MAX_PRE_SUM,
                  ACQ_MIN_SEGMENTS, ACQ_MAX_SEGMENTS);
        return XRIT_E_INVALID;
    }
    return stage_create(out, device, [&](xrit_acquire &aq) {
        aq.par = par;
        XR_TRY(aq.state.reserve(sizeof(xrit_acquire_state)));
        XR_TRY(aq.tables.reserve(ACQ_TABLE_BYTES));
        std::vector<float> t(ACQ_TABLE_BYTES / 4);
        const double step = 2.0 * 3.14159265358979323846 / (double)ACQ_N;
        for (unsigned k = 0; k < ACQ_N; ++k) {
            t[2 * k] = (float)std::cos(step * k);
            t[2 * k + 1] = (float)-std::sin(step * k);
            t[2 * ACQ_N + k] = (float)(0.5 - 0.5 * std::cos(step * k));
        }
        XR_TRY(aq.write_state(aq.tables.p, t.data(), ACQ_TABLE_BYTES));
        return xrit_acquire_reset(&aq);
    });
}

int xrit_acquire_destroy(xrit_acquire *aq) { return stage_destroy(aq); }

int xrit_acquire_reset(xrit_acquire *aq)
{
    if (!aq) { set_error("null argument"); return XRIT_E_INVALID; }
    return aq->write_state(aq->state.p, nullptr, sizeof(xrit_acquire_state));
}

int xrit_acquire_set_frequency(xrit_acquire *aq, double hz)
{
    if (!aq) { set_error("null argument"); return XRIT_E_INVALID; }
    int64_t inc;
    if (!acquire_inc_from_hz(hz, aq->par.sample_rate, inc)) {
        set_error("acquire: |hz| must be below half the sample rate (%g)", aq->par.sample_rate);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(aq->device));
    return launch_acquire_set_inc(aq->st(), (long long)inc, aq->last_stream);
}

static int check_samples(const xrit_acquire *aq, const void *samples, size_t n, int type, const void *out)
{
    if (!aq || !out || (n && !samples)) { set_error("null argument"); return XRIT_E_INVALID; }
    const size_t bytes = acquire_sample_bytes(type);
    if (!bytes) {
        set_error("acquire: sample type %d (FLOATIQ, S16IQ and S8IQ are taken; U8IQ's DC tracker belongs to the chain's ingest)", type);
        return XRIT_E_INVALID;
    }
    if (n > ACQ_MAX_SAMPLES) { set_error("acquire: at most %zu samples per call", ACQ_MAX_SAMPLES); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static int estimate_run(xrit_acquire *aq, const void *d_samples, size_t n, int type, int apply, xrit_acquire_estimate_record *d_record,
                        hipStream_t s)
{
    const unsigned segments = acquire_segments(n, aq->par.pre_sum, aq->par.segments);
    AcquireScratch sc;
    XR_TRY(aq->scratch.reserve(acquire_scratch_carve(nullptr, segments, sc)));
    acquire_scratch_carve(aq->scratch.p, segments, sc);
    XR_TRY(launch_acquire_estimate(d_samples, type, segments, aq->par, aq->tw(), aq->win(), sc, apply, aq->st(), d_record, s));
    aq->ran_on(s);
    return XRIT_OK;
}

int xrit_acquire_estimate_device(xrit_acquire *aq, const void *d_samples, size_t n_complex, int sample_type, int apply,
                                 xrit_acquire_estimate_record *d_record, void *stream)
{
    XR_TRY(check_samples(aq, d_samples, n_complex, sample_type, d_record));
    if (((size_t)d_samples % acquire_sample_bytes(sample_type)) || ((size_t)d_record & 7)) {
        set_error("acquire: the samples must be aligned to one complex sample, the record to 8 bytes");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(aq->device));
    return estimate_run(aq, d_samples, n_complex, sample_type, apply, d_record, (hipStream_t)stream);
}

int xrit_acquire_mix_device(xrit_acquire *aq, const void *d_samples, size_t n_complex, int sample_type, float *d_out, void *stream)
{
    XR_TRY(check_samples(aq, d_samples, n_complex, sample_type, n_complex ? (const void *)d_out : (const void *)aq));
    if (((size_t)d_samples % acquire_sample_bytes(sample_type)) || ((size_t)d_out & 7)) {
        set_error("acquire: the samples must be aligned to one complex sample, the output to 8 bytes");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(aq->device));
    XR_TRY(launch_acquire_mix(d_samples, sample_type, n_complex, reinterpret_cast<float2 *>(d_out), aq->st(), (hipStream_t)stream));
    aq->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

// the samples of a host-buffer call in h_in, on the own stream
static int upload(xrit_acquire *aq, const void *samples, size_t n, int type, hipStream_t &s)
{
    XR_TRY(aq->adopt_own_stream(s));
    const size_t bytes = n * acquire_sample_bytes(type);
    XR_TRY(aq->h_in.reserve(bytes + 16));
    if (bytes) XR_HIP(hipMemcpyAsync(aq->h_in.p, samples, bytes, hipMemcpyHostToDevice, s));
    return XRIT_OK;
}

int xrit_acquire_estimate(xrit_acquire *aq, const void *samples, size_t n_complex, int sample_type, int apply,
                          xrit_acquire_estimate_record *record)
{
    XR_TRY(check_samples(aq, samples, n_complex, sample_type, record));
    hipStream_t s;
    XR_TRY(upload(aq, samples, n_complex, sample_type, s));
    XR_TRY(aq->h_record.reserve(sizeof *record));
    XR_TRY(estimate_run(aq, aq->h_in.p, n_complex, sample_type, apply, aq->h_record.as<xrit_acquire_estimate_record>(), s));
    XR_HIP(hipMemcpyAsync(record, aq->h_record.p, sizeof *record, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_acquire_mix(xrit_acquire *aq, const void *samples, size_t n_complex, int sample_type, float *out)
{
    XR_TRY(check_samples(aq, samples, n_complex, sample_type, n_complex ? (const void *)out : (const void *)aq));
    hipStream_t s;
    XR_TRY(upload(aq, samples, n_complex, sample_type, s));
    XR_TRY(aq->h_out.reserve(n_complex * 8 + 16));
    XR_TRY(launch_acquire_mix(aq->h_in.p, sample_type, n_complex, aq->h_out.as<float2>(), aq->st(), s));
    aq->ran_on(s);
    if (n_complex) XR_HIP(hipMemcpyAsync(out, aq->h_out.p, n_complex * 8, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_acquire_get_state(xrit_acquire *aq, xrit_acquire_state *out)
{
    if (!aq || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    return aq->read_back(out, aq->st(), sizeof *out);
}
