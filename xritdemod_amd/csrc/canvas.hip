// canvas.hip -- the decoded lines of one files call and the images call on it, placed into the canvases of the images
// their segment files belong to (tests/canvas_spec.py is the serial statement; canvas_rule.h has the
// rule's predicates):
//  (a) head, one lane per record: a BEGINS rice record's headers walked for the segment identification and the
//      annotation (the walk of files.hip).
//  (b) rule, one wave: the records in order, 64 at a time.  The lanes load their records, ballot which ones the rule
//      has to look at, and the wave takes those one after the other: a lane per slot for the identity match and the
//      lowest free slot, a lane per segment for the rectangle test.  The only writer of key states, masks and segment
//      rectangles; lane s holds slot s in registers from the first record to the last.
//  (c) place, one wave per line: the one kernel that moves real bytes.
//  (d) commit, one wave per record: its lines counted (placed, clipped, faults) into its segment and its output.
//  (e) finish, one workgroup: the slots' sums and `complete`, the slot snapshot, the counters, the summary; the only
//      kernel that does anything in a refused call (overflow 2).
// Everything is integer; every launch is sized from the host's bounds and strides; the true counts are read from the
// two summaries on the device.
#include "canvas_rule.h"
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {

namespace {
constexpr unsigned WAVES = 4;           // per workgroup of the kernels that take a wave per item
constexpr unsigned SEGS = XRIT_CANVAS_MAX_SEGMENTS;
// the rule kernel's tallies of a call
enum { T_CANVASES = 0, T_BEGUN, T_DONE, T_ABORTED, T_REASON /* + reason - 2, six of them */, T_COUNT = T_REASON + 6 };

struct Counts { unsigned np, nf, nl; };

// the call's true counts; false: the call is refused
__device__ __forceinline__ bool canvas_counts(const xrit_files_summary *fs, const xrit_images_summary *is, const CanvasBounds &b, Counts &c)
{
    const unsigned long long p = fs->pieces, f = fs->files, l = is->lines;
    // (the two byte sizes bound every access instead: a first piece or a line that lies outside them is not read)
    const bool run = fs->overflow == 0 && is->overflow == 0 && p <= b.max_pieces && f <= b.max_files && l <= b.max_lines;
    c.np = run ? (unsigned)p : 0u;
    c.nf = run ? (unsigned)f : 0u;
    c.nl = run ? (unsigned)l : 0u;
    return run;
}

__device__ __forceinline__ bool key_ok(const xrit_file_record &r) { return r.vcid < NVC && r.apid < 2048; }
}  // namespace

// (a) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) canvas_head_kernel(const unsigned char *__restrict__ bytes, const xrit_file_piece *__restrict__ pieces,
                                                          const xrit_file_record *__restrict__ files,
                                                          const xrit_image_file *__restrict__ image_files,
                                                          const xrit_files_summary *__restrict__ fs, const xrit_images_summary *__restrict__ is,
                                                          CanvasBounds b, CanvasHead *__restrict__ heads)
{
    Counts c;
    if (!canvas_counts(fs, is, b, c)) return;
    for (unsigned f = blockIdx.x * 256u + threadIdx.x; f < c.nf; f += gridDim.x * 256u) {
        const xrit_file_record r = files[f];
        CanvasHead h{};
        if ((r.flags & XRIT_FILE_BEGINS) && image_files[f].rice) {
            const unsigned char *p = nullptr;
            unsigned n = 0;
            unsigned long long base = 0;
            if (r.n_pieces >= 1 && r.first_piece < c.np) {
                const xrit_file_piece pc = pieces[r.first_piece];
                if (pc.offset <= b.n_bytes && pc.length <= b.n_bytes - pc.offset) {
                    p = bytes + pc.offset;
                    n = pc.length;
                    base = pc.offset;
                }
            }
            h = canvas_walk(p, n, base, r.columns, r.lines);
        }
        heads[f] = h;
    }
}

// (b) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) canvas_rule_kernel(const unsigned char *__restrict__ bytes, const xrit_file_record *__restrict__ files,
                                                         const xrit_image_file *__restrict__ image_files,
                                                         const xrit_files_summary *__restrict__ fs, const xrit_images_summary *__restrict__ is,
                                                         CanvasBounds b, const CanvasHead *__restrict__ heads, xrit_canvas_slot *slots,
                                                         xrit_canvas_segment *segs, xrit_canvas_key_state *keys,
                                                         const xrit_canvas_counters *__restrict__ counters, unsigned n_slots,
                                                         unsigned long long slot_bytes, CanvasPlace *__restrict__ place,
                                                         unsigned long long *__restrict__ call)
{
    __shared__ unsigned tally[T_COUNT];
    const unsigned lane = threadIdx.x;
    Counts c;
    if (!canvas_counts(fs, is, b, c)) return;
    if (lane < T_COUNT) tally[lane] = 0;            // (lane 0 alone adds to them, behind this store in the wave's order)
    __syncthreads();
    const unsigned callno = (unsigned)(counters->calls + 1);
    // slot `lane`, in registers for the whole call
    const bool mine_exists = lane < n_slots;
    xrit_canvas_slot *S = slots + lane;             // (the table has 64 entries whatever n_slots is)
    bool in_use = mine_exists && S->in_use;
    unsigned s_vcid = S->vcid, s_bits = S->bits, s_image_id = S->image_id, s_max_column = S->max_column, s_max_row = S->max_row,
             s_max_segment = S->max_segment, s_pitch = S->pitch, s_born = S->born_call, s_touched = S->touched_call;
    const unsigned s_generation = S->generation;
    unsigned long long s_begun = S->begun_mask, s_done = S->done_mask, s_aborted = S->aborted_mask;

    for (unsigned base = 0; base < c.nf; base += 64) {
        const unsigned f = base + lane;
        xrit_file_record r{};
        CanvasHead h{};
        xrit_canvas_key_state k{};
        unsigned kind = 0, pre = 0;                 // 1: BEGINS, no rice; 2: BEGINS, rice; 3: rice without BEGINS
        if (f < c.nf) {
            r = files[f];
            const bool rice = image_files[f].rice != 0, begins = r.flags & XRIT_FILE_BEGINS;
            if (key_ok(r)) kind = begins ? (rice ? 2u : 1u) : (rice ? 3u : 0u);
            if (kind == 2) {
                h = heads[f];
                pre = canvas_check(h, r.columns, r.lines, r.bits_per_pixel, slot_bytes);
            }
            // (a record without BEGINS is the first of its key in a call: nothing in front of it rewrites the key)
            if (kind == 3) k = keys[(unsigned)r.vcid * 2048u + r.apid];
        }
        CanvasPlace mine{0, XRIT_CANVAS_NOT_RICE, 0, 0, 0, 0};
        unsigned long long todo = __ballot(kind != 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned kind_l = __shfl(kind, l, 64), vcid_l = __shfl((unsigned)r.vcid, l, 64), apid_l = __shfl((unsigned)r.apid, l, 64),
                           serial_l = __shfl(r.key_serial, l, 64), flags_l = __shfl((unsigned)r.flags, l, 64);
            CanvasPlace pl{-1, XRIT_CANVAS_NOT_RICE, 0, 0, 0, 0};
            unsigned generation_l = 0;
            if (kind_l == 2) {
                const unsigned bits_l = __shfl((unsigned)r.bits_per_pixel, l, 64), cols_l = __shfl((unsigned)r.columns, l, 64),
                               lines_l = __shfl((unsigned)r.lines, l, 64);
                CanvasHead hl;
                hl.image_id = __shfl(h.image_id, l, 64);
                hl.segment = __shfl(h.segment, l, 64);
                hl.start_column = __shfl(h.start_column, l, 64);
                hl.start_line = __shfl(h.start_line, l, 64);
                hl.max_segment = __shfl(h.max_segment, l, 64);
                hl.max_column = __shfl(h.max_column, l, 64);
                hl.max_row = __shfl(h.max_row, l, 64);
                hl.name_len = __shfl(h.name_len, l, 64);
                hl.name_off = __shfl(h.name_off, l, 64);
                pl.reason = __shfl(pre, l, 64);
                if (!pl.reason) {
                    const unsigned long long same = __ballot(canvas_same(in_use, s_vcid, s_bits, s_image_id, s_max_column, s_max_row,
                                                                         s_max_segment, vcid_l, bits_l, hl));
                    const unsigned long long free_slots = __ballot(mine_exists && !in_use);
                    const unsigned long long bit = 1ull << (hl.segment - 1);
                    int slot = -1;
                    bool born = false;
                    if (same) {
                        slot = __ffsll((long long)same) - 1;
                        if (__shfl(s_begun, slot, 64) & bit)
                            pl.reason = XRIT_CANVAS_DUPLICATE;
                        else if (__ballot(canvas_rects_meet(segs[(unsigned)slot * SEGS + lane], hl.start_line, lines_l, hl.start_column, cols_l)))
                            pl.reason = XRIT_CANVAS_OVERLAP;
                    } else if (free_slots) {
                        slot = __ffsll((long long)free_slots) - 1;
                        born = true;
                    } else
                        pl.reason = XRIT_CANVAS_NO_SLOT;
                    if (!pl.reason) {
                        if ((int)lane == slot) {
                            if (born) {
                                in_use = true;
                                s_vcid = vcid_l;
                                s_bits = bits_l;
                                s_image_id = hl.image_id;
                                s_max_column = hl.max_column;
                                s_max_row = hl.max_row;
                                s_max_segment = hl.max_segment;
                                s_pitch = canvas_pitch(hl.max_column, bits_l);
                                s_born = callno;
                            }
                            s_begun |= bit;
                        }
                        // (a free slot is all zero, so is its name: the bytes behind the text stay as they are)
                        if (born && lane < hl.name_len) slots[slot].name[lane] = bytes[hl.name_off + lane];
                        if (lane == 0) {
                            xrit_canvas_segment g{};
                            g.start_line = hl.start_line;
                            g.start_column = hl.start_column;
                            g.lines = lines_l;
                            g.columns = cols_l;
                            g.key_serial = serial_l;
                            g.apid = (uint16_t)apid_l;
                            g.begun = 1;
                            segs[(unsigned)slot * SEGS + hl.segment - 1] = g;
                            tally[T_BEGUN] += 1;
                            tally[T_CANVASES] += born;
                        }
                        pl = CanvasPlace{slot, XRIT_CANVAS_PLACED, hl.segment, hl.start_line, hl.start_column, lines_l};
                        generation_l = __shfl(s_generation, slot, 64);
                        // the rectangle is in memory before a later record's lanes load that table
                        __threadfence_block();
                    }
                }
            } else if (kind_l == 3) {
                xrit_canvas_key_state kl;
                kl.key_serial = __shfl(k.key_serial, l, 64);
                kl.slot = __shfl(k.slot, l, 64);
                kl.generation = __shfl(k.generation, l, 64);
                kl.segment = __shfl(k.segment, l, 64);
                kl.start_line = __shfl(k.start_line, l, 64);
                kl.start_column = __shfl(k.start_column, l, 64);
                kl.lines = __shfl(k.lines, l, 64);
                kl.placed = (uint8_t)__shfl((unsigned)k.placed, l, 64);
                // canvas_continues on the registers: generations change at a release alone, between calls
                const bool ok = kl.placed && kl.key_serial == serial_l && kl.slot < n_slots && kl.segment >= 1 && kl.segment <= SEGS &&
                                __shfl((unsigned)in_use, kl.slot & 63u, 64) && __shfl(s_generation, kl.slot & 63u, 64) == kl.generation;
                pl = ok ? CanvasPlace{(int)kl.slot, XRIT_CANVAS_PLACED, kl.segment, kl.start_line, kl.start_column, kl.lines}
                        : CanvasPlace{-1, XRIT_CANVAS_NO_PLACEMENT, 0, 0, 0, 0};
            }
            if (kind_l != 3 && lane == 0) keys[vcid_l * 2048u + apid_l] = canvas_key_of(serial_l, pl, generation_l);
            if (pl.reason == XRIT_CANVAS_PLACED) {
                const unsigned long long bit = 1ull << (pl.segment - 1);
                if ((int)lane == pl.slot) {
                    s_touched = callno;
                    if (flags_l & XRIT_FILE_ENDS) s_done |= bit;
                    if (flags_l & XRIT_FILE_ABORTED) s_aborted |= bit;
                }
                if (lane == 0) {
                    tally[T_DONE] += (flags_l & XRIT_FILE_ENDS) != 0;
                    tally[T_ABORTED] += (flags_l & XRIT_FILE_ABORTED) != 0;
                }
            } else if (pl.reason >= XRIT_CANVAS_BAD_SEGMENT && lane == 0)
                tally[T_REASON + pl.reason - XRIT_CANVAS_BAD_SEGMENT] += 1;
            if ((int)lane == l) mine = pl;
        }
        if (f < c.nf) place[f] = mine;
    }
    if (mine_exists) {
        S->in_use = in_use;
        S->vcid = (uint8_t)s_vcid;
        S->bits = (uint8_t)s_bits;
        S->image_id = s_image_id;
        S->max_column = s_max_column;
        S->max_row = s_max_row;
        S->max_segment = s_max_segment;
        S->pitch = s_pitch;
        S->born_call = s_born;
        S->touched_call = s_touched;
        S->begun_mask = s_begun;
        S->done_mask = s_done;
        S->aborted_mask = s_aborted;
    }
    __syncthreads();
    if (lane < T_COUNT) call[lane] = tally[lane];
}

// (c) ------------------------------------------------------------------------------------------------------------------
// No two lines ever write one pixel -- one file per (canvas, segment), the segments' rectangles disjoint, `row` unique
// within a file: the rule guarantees it -- so plain stores in any order give the same canvas, without atomics.
__global__ void __launch_bounds__(64 * WAVES) canvas_place_kernel(const unsigned char *__restrict__ image_bytes,
                                                                  const xrit_image_line *__restrict__ lines,
                                                                  const xrit_image_file *__restrict__ image_files,
                                                                  const xrit_files_summary *__restrict__ fs,
                                                                  const xrit_images_summary *__restrict__ is, CanvasBounds b,
                                                                  const CanvasPlace *__restrict__ place, const xrit_canvas_slot *__restrict__ slots,
                                                                  unsigned char *__restrict__ pixels, unsigned long long slot_bytes)
{
    const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
    Counts c;
    if (!canvas_counts(fs, is, b, c)) return;
    for (unsigned i = wave; i < c.nl; i += n_waves) {
        const xrit_image_line ln = lines[i];
        const unsigned f = ln.file;
        if (f >= c.nf) continue;
        const CanvasPlace pl = place[f];
        if (pl.reason != XRIT_CANVAS_PLACED || i - image_files[f].first_line >= image_files[f].n_lines) continue;
        const xrit_canvas_slot *s = slots + pl.slot;
        uint64_t at;
        if (!canvas_line_dst(ln.offset, ln.length, ln.row, pl, s->pitch, s->max_row, s->bits, b.n_image_bytes, at)) continue;
        const unsigned char *src = image_bytes + ln.offset;
        unsigned char *dst = pixels + (unsigned long long)pl.slot * slot_bytes + at;
        const unsigned length = ln.length;
        const size_t both = (size_t)src | (size_t)dst;
        if (!(both & 3)) {
            unsigned done = 0;
            if (!(both & 15)) {
                const unsigned n16 = length >> 4;
                for (unsigned j = lane; j < n16; j += 64) reinterpret_cast<uint4 *>(dst)[j] = reinterpret_cast<const uint4 *>(src)[j];
                done = n16 << 4;
            }
            const unsigned n4 = (length - done) >> 2;
            for (unsigned j = lane; j < n4; j += 64)
                reinterpret_cast<unsigned *>(dst + done)[j] = reinterpret_cast<const unsigned *>(src + done)[j];
            done += n4 << 2;
            if (lane < length - done) dst[done + lane] = src[done + lane];
        } else if (!((size_t)src & 3)) {
            // the destination is not aligned (start_column * width is odd or 2 mod 4): dword loads, byte stores, a byte tail
            const unsigned n4 = length >> 2;
            for (unsigned j = lane; j < n4; j += 64) {
                const unsigned v = reinterpret_cast<const unsigned *>(src)[j];
                unsigned char *d = dst + 4u * j;
                d[0] = (unsigned char)v;
                d[1] = (unsigned char)(v >> 8);
                d[2] = (unsigned char)(v >> 16);
                d[3] = (unsigned char)(v >> 24);
            }
            if (lane < (length & 3u)) dst[4u * n4 + lane] = src[4u * n4 + lane];
        } else
            for (unsigned j = lane; j < length; j += 64) dst[j] = src[j];
    }
}

// (d) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * WAVES) canvas_commit_kernel(const xrit_image_line *__restrict__ lines,
                                                                   const xrit_image_file *__restrict__ image_files,
                                                                   const xrit_files_summary *__restrict__ fs,
                                                                   const xrit_images_summary *__restrict__ is, CanvasBounds b,
                                                                   const CanvasPlace *__restrict__ place, const xrit_canvas_slot *__restrict__ slots,
                                                                   xrit_canvas_segment *__restrict__ segs, xrit_canvas_file *__restrict__ canvas_files)
{
    const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
    Counts c;
    if (!canvas_counts(fs, is, b, c)) return;
    for (unsigned f = wave; f < c.nf; f += n_waves) {
        const CanvasPlace pl = place[f];
        const xrit_image_file fl = image_files[f];
        xrit_canvas_file o{};
        if (fl.rice && pl.reason != XRIT_CANVAS_NOT_RICE) {
            o.slot = pl.slot;
            o.reason = pl.reason;
        }
        if (o.reason == XRIT_CANVAS_PLACED) {
            const xrit_canvas_slot *s = slots + pl.slot;
            const unsigned pitch = s->pitch, max_row = s->max_row, bits = s->bits;
            unsigned placed = 0, clipped = 0, faults = 0;
            for (unsigned j = lane; j < fl.n_lines && fl.first_line + j < c.nl; j += 64) {
                const xrit_image_line ln = lines[fl.first_line + j];
                uint64_t at;
                const bool fits = canvas_line_dst(ln.offset, ln.length, ln.row, pl, pitch, max_row, bits, b.n_image_bytes, at);
                placed += fits;
                clipped += !fits;
                faults += fits && ln.status != 0;
            }
            placed = wave_sum(placed);
            clipped = wave_sum(clipped);
            faults = wave_sum(faults);
            o.segment = pl.segment;
            o.start_line = pl.start_line;
            o.start_column = pl.start_column;
            o.lines_placed = placed;
            o.lines_clipped = clipped;
            o.faults = faults;
            // (one record per (canvas, segment) in a call: its file's)
            if (lane == 0) {
                xrit_canvas_segment *g = segs + (unsigned)pl.slot * SEGS + pl.segment - 1;
                g->placed += placed;
                g->faults += faults;
            }
        }
        if (lane == 0) canvas_files[f] = o;
    }
}

// (e) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) canvas_finish_kernel(const xrit_files_summary *__restrict__ fs, const xrit_images_summary *__restrict__ is,
                                                            CanvasBounds b, const xrit_canvas_file *__restrict__ canvas_files,
                                                            const unsigned long long *__restrict__ call, xrit_canvas_slot *slots,
                                                            const xrit_canvas_segment *__restrict__ segs, unsigned n_slots,
                                                            xrit_canvas_counters *__restrict__ counters, xrit_canvas_slot *__restrict__ out_slots,
                                                            xrit_canvas_summary *__restrict__ sum)
{
    __shared__ unsigned long long s_sum[4][4];
    __shared__ unsigned s_completed[XRIT_CANVAS_MAX_SLOTS];
    const unsigned tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    Counts c;
    const bool run = canvas_counts(fs, is, b, c);
    if (tid < XRIT_CANVAS_MAX_SLOTS) s_completed[tid] = 0;
    __syncthreads();
    if (run) {
        for (unsigned s = w; s < n_slots; s += 4) {
            if (!slots[s].in_use) continue;
            const unsigned placed = wave_sum(segs[s * SEGS + lane].placed), faults = wave_sum(segs[s * SEGS + lane].faults);
            if (lane == 0) {
                const unsigned m = slots[s].max_segment;
                const bool complete = slots[s].done_mask == (m >= 64 ? ~0ull : (1ull << m) - 1);
                s_completed[s] = complete && !slots[s].complete;
                slots[s].lines_placed = placed;
                slots[s].faults = faults;
                slots[s].complete = complete;
            }
        }
    }
    unsigned long long v[4] = {0, 0, 0, 0};         // records placed, their lines placed, clipped, faults
    for (unsigned f = tid; f < c.nf; f += 256u) {
        const xrit_canvas_file o = canvas_files[f];
        if (o.reason != XRIT_CANVAS_PLACED) continue;
        v[0] += 1;
        v[1] += o.lines_placed;
        v[2] += o.lines_clipped;
        v[3] += o.faults;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        v[u] = wave_sum(v[u]);
        if (lane == 0) s_sum[w][u] = v[u];
    }
    __syncthreads();
    if (run) {
        // the slot table after the call
        const unsigned words = n_slots * (unsigned)(sizeof(xrit_canvas_slot) / 4);
        for (unsigned i = tid; i < words; i += 256u) reinterpret_cast<unsigned *>(out_slots)[i] = reinterpret_cast<const unsigned *>(slots)[i];
    }
    if (tid != 0) return;
    xrit_canvas_counters t = *counters;
    xrit_canvas_summary o{};
    if (run) {
        for (int u = 0; u < 4; ++u) v[u] = s_sum[0][u] + s_sum[1][u] + s_sum[2][u] + s_sum[3][u];
        unsigned completed = 0;
        for (unsigned s = 0; s < n_slots; ++s) completed += s_completed[s];
        o.placed = v[0];
        o.call_lines_placed = v[1];
        o.call_lines_clipped = v[2];
        o.call_faults = v[3];
        o.completed = completed;
        t.calls += 1;
        t.canvases_begun += call[T_CANVASES];
        t.canvases_completed += completed;
        t.segments_begun += call[T_BEGUN];
        t.segments_done += call[T_DONE];
        t.segments_aborted += call[T_ABORTED];
        t.lines_placed += v[1];
        t.lines_clipped += v[2];
        t.faults += v[3];
        t.bad_segment += call[T_REASON + 0];
        t.too_large += call[T_REASON + 1];
        t.duplicate += call[T_REASON + 2];
        t.overlap += call[T_REASON + 3];
        t.no_slot += call[T_REASON + 4];
        t.no_placement += call[T_REASON + 5];
        *counters = t;
    }
    o.calls = t.calls;
    o.canvases_begun = t.canvases_begun;
    o.canvases_completed = t.canvases_completed;
    o.segments_begun = t.segments_begun;
    o.segments_done = t.segments_done;
    o.segments_aborted = t.segments_aborted;
    o.lines_placed = t.lines_placed;
    o.lines_clipped = t.lines_clipped;
    o.faults = t.faults;
    o.bad_segment = t.bad_segment;
    o.too_large = t.too_large;
    o.duplicate = t.duplicate;
    o.overlap = t.overlap;
    o.no_slot = t.no_slot;
    o.no_placement = t.no_placement;
    o.overflow = run ? 0u : 2u;
    *sum = o;
}

// a slot free again: its record and its segments zero, the generation one more
__global__ void __launch_bounds__(256) canvas_release_kernel(xrit_canvas_slot *slots, xrit_canvas_segment *segs, unsigned slot)
{
    __shared__ unsigned s_generation;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_generation = slots[slot].generation + 1u;
    __syncthreads();
    unsigned *s = reinterpret_cast<unsigned *>(slots + slot), *g = reinterpret_cast<unsigned *>(segs + slot * SEGS);
    for (unsigned i = tid; i < sizeof(xrit_canvas_slot) / 4; i += 256u) s[i] = 0;
    for (unsigned i = tid; i < SEGS * sizeof(xrit_canvas_segment) / 4; i += 256u) g[i] = 0;
    __syncthreads();
    if (tid == 0) slots[slot].generation = s_generation;
}

size_t canvas_scratch_carve(void *base, size_t max_files_in, CanvasScratch &sc)
{
    const size_t R = max_files_in ? max_files_in : 1;
    Carver c{static_cast<char *>(base)};
    sc.heads = c.take<CanvasHead>(R, 16);
    sc.place = c.take<CanvasPlace>(R, 16);
    sc.call = c.take<unsigned long long>(T_COUNT, 16);
    return c.used();
}

int launch_canvas(const unsigned char *bytes, const xrit_file_piece *pieces, const xrit_file_record *files, const xrit_files_summary *fsum,
                  const unsigned char *image_bytes, const xrit_image_line *lines, const xrit_image_file *image_files,
                  const xrit_images_summary *isum, const CanvasBounds &b, const CanvasState &st, CanvasScratch &sc,
                  xrit_canvas_file *canvas_files, xrit_canvas_slot *out_slots, xrit_canvas_summary *summary, hipStream_t s)
{
    const size_t R = b.max_files ? b.max_files : 1, L = b.max_lines ? b.max_lines : 1;
    // (the counts are on the device: grids no larger than fill the chip a few times over, striding)
    const unsigned g_head = div_up(R, 256), g_line = div_up(L, WAVES), g_rec = div_up(R, WAVES);
    hipLaunchKernelGGL(canvas_head_kernel, dim3(g_head < 1024u ? g_head : 1024u), dim3(256), 0, s, bytes, pieces, files, image_files, fsum,
                       isum, b, sc.heads);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(canvas_rule_kernel, dim3(1), dim3(64), 0, s, bytes, files, image_files, fsum, isum, b, sc.heads, st.slots, st.segs,
                       st.keys, st.counters, st.n_slots, (unsigned long long)st.slot_bytes, sc.place, sc.call);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(canvas_place_kernel, dim3(g_line < 8192u ? g_line : 8192u), dim3(64 * WAVES), 0, s, image_bytes, lines, image_files,
                       fsum, isum, b, sc.place, st.slots, st.pixels, (unsigned long long)st.slot_bytes);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(canvas_commit_kernel, dim3(g_rec < 4096u ? g_rec : 4096u), dim3(64 * WAVES), 0, s, lines, image_files, fsum, isum, b,
                       sc.place, st.slots, st.segs, canvas_files);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(canvas_finish_kernel, dim3(1), dim3(256), 0, s, fsum, isum, b, canvas_files, sc.call, st.slots, st.segs, st.n_slots,
                       st.counters, out_slots, summary);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_canvas_release(const CanvasState &st, unsigned slot, hipStream_t s)
{
    XR_HIP(hipMemsetAsync(st.pixels + (size_t)slot * st.slot_bytes, 0, st.slot_bytes, s));
    hipLaunchKernelGGL(canvas_release_kernel, dim3(1), dim3(256), 0, s, st.slots, st.segs, slot);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
