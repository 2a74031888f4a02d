// monitor.cpp -- C ABI of the link monitor (include/xritdemod_amd.h, "Link monitor"): the handle owns the state (one
// xrit_monitor_state) and two scratch records in device memory, and keeps the open block's fill on the host so that the rows
// of a push are known without a read-back; the kernels are in monitor.hip, the plain host parts in monitor_host.h.
#include <cstddef>

#include "common.h"
#include "kernels.h"
#include "monitor_host.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_monitor_block) == 64 && offsetof(xrit_monitor_block, s1) == 16 && offsetof(xrit_monitor_block, sum) == 40 &&
                  offsetof(xrit_monitor_block, sat) == 48,
              "xrit_monitor_block layout (MONITOR_BLOCK_DTYPE mirrors it)");
static_assert(sizeof(xrit_monitor_summary) == 32, "xrit_monitor_summary layout (MONITOR_SUMMARY_DTYPE mirrors it)");
static_assert(sizeof(xrit_monitor_state) == 2144 && offsetof(xrit_monitor_state, symbols_total) == 64 && offsetof(xrit_monitor_state, last_neg) == 88 &&
                  offsetof(xrit_monitor_state, hist) == 96,
              "xrit_monitor_state layout (MONITOR_STATE_DTYPE mirrors it)");
static_assert(sizeof(xrit_monitor_quality) == 64 && offsetof(xrit_monitor_quality, flags) == 56, "xrit_monitor_quality layout");

struct xrit_monitor : StageHandle {
    uint32_t block = 0;
    int type = 0;
    uint32_t open_n = 0;                            // symbols_total mod block, moved on by every push that was enqueued
    DevBuf state, parts;
    DevBuf h_in, h_rows;                            // the host-buffer form's
    xrit_monitor_state *st() const { return state.as<xrit_monitor_state>(); }
    void close_all() { close({&state, &parts, &h_in, &h_rows}); }
};

int xrit_monitor_create(xrit_monitor **out, uint32_t block, int symbol_type, int device)
{
    if (!out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    if (block == 0) block = MON_DEFAULT_BLOCK;
    if (!monitor_block_ok(block) || !monitor_symbol_bytes(symbol_type)) {
        set_error("monitor: block a multiple of 64 in %u .. %u (0 selects %u), symbol type XRIT_SYMBOL_F32 or XRIT_SYMBOL_I8", MON_MIN_BLOCK,
                  MON_MAX_BLOCK, MON_DEFAULT_BLOCK);
        return XRIT_E_INVALID;
    }
    return stage_create(out, device, [&](xrit_monitor &m) {
        m.block = block;
        m.type = symbol_type;
        XR_TRY(m.state.reserve(sizeof(xrit_monitor_state)));
        XR_TRY(m.parts.reserve(2 * sizeof(xrit_monitor_block)));
        return xrit_monitor_reset(&m);
    });
}

int xrit_monitor_destroy(xrit_monitor *m) { return stage_destroy(m); }

int xrit_monitor_reset(xrit_monitor *m)
{
    if (!m) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(m->write_state(m->state.p, nullptr, sizeof(xrit_monitor_state)));
    m->open_n = 0;
    return XRIT_OK;
}

size_t xrit_monitor_rows(const xrit_monitor *m, size_t n)
{
    if (!m || n > MON_MAX_SYMBOLS) return 0;
    return monitor_plan(m->block, m->open_n, n).rows;
}

// everything a push checks before anything is enqueued
static int check_push(const xrit_monitor *m, const void *symbols, size_t n, const void *rows, size_t cap_rows, MonitorPlan &plan)
{
    if (!m || (n && !symbols)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (n > MON_MAX_SYMBOLS) { set_error("monitor: at most %zu symbols per push", MON_MAX_SYMBOLS); return XRIT_E_INVALID; }
    plan = monitor_plan(m->block, m->open_n, n);
    if (cap_rows < plan.rows) {
        set_error("monitor: %zu blocks completed, room for %zu: the output buffer is too small", plan.rows, cap_rows);
        return XRIT_E_CAPACITY;
    }
    if (plan.rows && !rows) { set_error("null argument"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static int push_run(xrit_monitor *m, const void *d_symbols, const MonitorPlan &plan, xrit_monitor_block *d_rows, xrit_monitor_summary *d_summary,
                    hipStream_t s)
{
    XR_TRY(launch_monitor_push(d_symbols, m->type, plan, m->parts.as<xrit_monitor_block>(), m->st(), d_rows, d_summary, s));
    m->ran_on(s);
    m->open_n = plan.open_after;
    return XRIT_OK;
}

int xrit_monitor_push_device(xrit_monitor *m, const void *d_symbols, size_t n, xrit_monitor_block *d_rows, size_t cap_rows,
                             xrit_monitor_summary *d_summary, void *stream)
{
    MonitorPlan plan;
    XR_TRY(check_push(m, d_symbols, n, d_rows, cap_rows, plan));
    if (((size_t)d_symbols % monitor_symbol_bytes(m->type)) || ((size_t)d_rows & 7) || ((size_t)d_summary & 7)) {
        set_error("monitor: the symbols must be aligned to one symbol, the rows and the summary to 8 bytes");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(m->device));
    return push_run(m, d_symbols, plan, d_rows, d_summary, (hipStream_t)stream);
}

int xrit_monitor_push(xrit_monitor *m, const void *symbols, size_t n, xrit_monitor_block *rows, size_t cap_rows, size_t *n_rows)
{
    MonitorPlan plan{};
    const int rc = check_push(m, symbols, n, rows, cap_rows, plan);
    if (n_rows) *n_rows = rc == XRIT_OK || rc == XRIT_E_CAPACITY ? plan.rows : 0;
    XR_TRY(rc);
    hipStream_t s;
    XR_TRY(m->adopt_own_stream(s));
    const size_t bytes = n * monitor_symbol_bytes(m->type);
    XR_TRY(m->h_in.reserve(bytes + 16));
    XR_TRY(m->h_rows.reserve((plan.rows + 1) * sizeof(xrit_monitor_block)));
    if (bytes) XR_HIP(hipMemcpyAsync(m->h_in.p, symbols, bytes, hipMemcpyHostToDevice, s));
    XR_TRY(push_run(m, m->h_in.p, plan, m->h_rows.as<xrit_monitor_block>(), nullptr, s));
    if (plan.rows) XR_HIP(hipMemcpyAsync(rows, m->h_rows.p, plan.rows * sizeof(xrit_monitor_block), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_monitor_get_state(xrit_monitor *m, xrit_monitor_state *out)
{
    if (!m || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    return m->read_back(out, m->st(), sizeof *out);
}

int xrit_monitor_derive(const xrit_monitor_block *b, int symbol_type, xrit_monitor_quality *q)
{
    if (!b || !q) { set_error("null argument"); return XRIT_E_INVALID; }
    const int rc = monitor_derive(*b, symbol_type, *q);
    if (rc != XRIT_OK) set_error("monitor: a record of n = 1 .. %u symbols of type XRIT_SYMBOL_F32 or XRIT_SYMBOL_I8, with sums that n lattice values give", MON_MAX_BLOCK);
    return rc;
}
