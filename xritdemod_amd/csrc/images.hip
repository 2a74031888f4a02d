// images.hip -- every Rice-coded line of every image file of one files call, decoded in one pass (DESIGN.md section 19;
// tests/image_spec.py is the serial statement).  The decision per record depends on the record, its first piece and the
// key's state alone (image_rule.h), so:
//  (a) mark, one lane per record: the rule -- most records are not images and cost one load -- and the record's line
//      and padded byte counts.  The only reader of the keys' state.
//  (b) scan, two levels over the records: per tile of 1024 records the exclusive prefix of lines and bytes inside the
//      tile and the tile's sums (the counter increments among them, by ballots); then one wave over the tiles: every
//      tile's base and the call's sums.
//  (c) decode, one wave per piece: the piece's `file` names its record; from the record's prefix and the piece's place in
//      it the wave knows its line index and output offset (or that it is no line and returns) and runs the wave form of
//      the Rice decoder (rice_core.h) with that record's (n, J, S).  The status goes to scratch per piece, so that a line
//      without room is still counted.
//  (d) commit, one wave per record: the fault tally of its lines, the xrit_image_file, and -- by the last record of a
//      key -- the key's new state; then one workgroup: the faults' sum, the counters, the summary.
// Everything is integer; every launch is sized from the host's bounds and strides; the true counts are read from the
// files summary on the device.  A refused call (overflow 2) runs (d)'s last kernel alone in effect: the others return.
#include "image_rule.h"
#include "kernels.h"
#include "rice_core.h"
#include "wave_ops.h"

namespace xrit {

namespace {
constexpr unsigned WAVES = 4;           // per workgroup of the kernels that take a wave per item

// the call's true counts; false: the call is refused
__device__ __forceinline__ bool images_counts(const xrit_files_summary *fs, unsigned long long max_pieces_in, unsigned long long max_files_in,
                                              unsigned &np, unsigned &nf)
{
    const unsigned long long p = fs->pieces, f = fs->files;
    const bool run = fs->overflow == 0 && p <= max_pieces_in && f <= max_files_in;
    np = run ? (unsigned)p : 0u;
    nf = run ? (unsigned)f : 0u;
    return run;
}
}  // namespace

// (a) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) images_mark_kernel(const xrit_file_piece *__restrict__ pieces, unsigned long long max_pieces_in,
                                                          const xrit_file_record *__restrict__ files, unsigned long long max_files_in,
                                                          const xrit_files_summary *__restrict__ fs, const xrit_image_key *__restrict__ keys,
                                                          ImageMark *__restrict__ mark, unsigned *__restrict__ rlines,
                                                          unsigned long long *__restrict__ rbytes)
{
    unsigned np, nf;
    if (!images_counts(fs, max_pieces_in, max_files_in, np, nf)) return;
    for (unsigned f = blockIdx.x * 256u + threadIdx.x; f < nf; f += gridDim.x * 256u) {
        const xrit_file_record r = files[f];
        // (a record whose pieces are not all among the call's is nobody's image)
        const bool inside = r.first_piece <= np && r.n_pieces <= np - r.first_piece;
        unsigned flen = 0, fidx = 0;
        if (inside && r.n_pieces) {
            flen = pieces[r.first_piece].length;
            fidx = pieces[r.first_piece].index_in_file;
        }
        xrit_image_key k{};
        if (!(r.flags & XRIT_FILE_BEGINS) && r.vcid < NVC && r.apid < 2048) k = keys[(unsigned)r.vcid * 2048u + r.apid];
        ImageMark m = image_mark(r, flen, fidx, k);
        if (!inside || r.vcid >= NVC || r.apid >= 2048) m = ImageMark{};
        mark[f] = m;
        rlines[f] = m.n_lines;
        rbytes[f] = (unsigned long long)m.n_lines * m.padded;
    }
}

// (b) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(IMAGES_TILE) images_tile_kernel(const xrit_files_summary *__restrict__ fs, unsigned long long max_pieces_in,
                                                                  unsigned long long max_files_in, const ImageMark *__restrict__ mark,
                                                                  unsigned *__restrict__ rlines, unsigned long long *__restrict__ rbytes,
                                                                  unsigned long long *__restrict__ tsum)
{
    constexpr unsigned NW = IMAGES_TILE / 64;
    __shared__ unsigned long long s_l[NW], s_b[NW];
    __shared__ unsigned s_c[NW][4];
    const unsigned tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    unsigned np, nf;
    if (!images_counts(fs, max_pieces_in, max_files_in, np, nf)) return;
    for (unsigned t = blockIdx.x; (unsigned long long)t * IMAGES_TILE < nf; t += gridDim.x) {
        const unsigned f = t * IMAGES_TILE + tid;
        const bool in = f < nf;
        const unsigned l = in ? rlines[f] : 0u;
        const unsigned long long b = in ? rbytes[f] : 0ull;
        const unsigned rice = in ? mark[f].rice : 0u, ev = in ? mark[f].events : 0u;
        const unsigned c_img = __popcll(__ballot(rice != 0)), c_beg = __popcll(__ballot((ev & IMAGE_BEGUN) != 0)),
                       c_end = __popcll(__ballot((ev & IMAGE_COMPLETED) != 0)), c_abt = __popcll(__ballot((ev & IMAGE_ABORTED) != 0));
        if (lane == 63) {
            s_c[w][0] = c_img;
            s_c[w][1] = c_beg;
            s_c[w][2] = c_end;
            s_c[w][3] = c_abt;
        }
        // (the tile's sum of lines in 64 bits: records given by hand may each claim all of the call's pieces)
        unsigned long long al, ab;
        const unsigned el = (unsigned)(block_incl_scan<NW>((unsigned long long)l, lane, w, s_l, al) - l);
        const unsigned long long eb = block_incl_scan<NW>(b, lane, w, s_b, ab) - b;
        if (in) {
            rlines[f] = el;
            rbytes[f] = eb;
        }
        unsigned long long *ts = tsum + (size_t)t * IMAGES_TSUM;
        if (tid == 0) {
            ts[0] = al;
            ts[1] = ab;
        }
        if (tid < 4) {
            unsigned long long c = 0;
            for (unsigned i = 0; i < NW; ++i) c += s_c[i][tid];
            ts[2 + tid] = c;
        }
        __syncthreads();
    }
}

// one wave over the tiles, 64 at a time: every tile's first line index and byte offset; the call's sums
__global__ void __launch_bounds__(64) images_total_kernel(const xrit_files_summary *__restrict__ fs, unsigned long long max_pieces_in,
                                                          unsigned long long max_files_in, const unsigned long long *__restrict__ tsum,
                                                          unsigned long long *__restrict__ tbase, unsigned long long *__restrict__ call)
{
    const unsigned lane = threadIdx.x;
    unsigned np, nf;
    if (!images_counts(fs, max_pieces_in, max_files_in, np, nf)) return;
    const unsigned T = (nf + IMAGES_TILE - 1) / IMAGES_TILE;
    unsigned long long carry[IMAGES_TSUM] = {0, 0, 0, 0, 0, 0};
    for (unsigned base = 0; base < T; base += 64) {
        const unsigned t = base + lane;
#pragma unroll
        for (unsigned u = 0; u < IMAGES_TSUM; ++u) {
            const unsigned long long before = wave_excl_scan_step(t < T ? tsum[(size_t)t * IMAGES_TSUM + u] : 0ull, lane, carry[u]);
            if (u < 2 && t < T) tbase[(size_t)t * 2 + u] = before;
        }
    }
    if (lane == 0)
        for (unsigned u = 0; u < IMAGES_TSUM; ++u) call[u] = carry[u];
}

// (c) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * WAVES) images_decode_kernel(const unsigned char *__restrict__ bytes, unsigned long long n_bytes,
                                                                   const xrit_file_piece *__restrict__ pieces, unsigned long long max_pieces_in,
                                                                   const xrit_file_record *__restrict__ files, unsigned long long max_files_in,
                                                                   const xrit_files_summary *__restrict__ fs, const ImageMark *__restrict__ mark,
                                                                   const unsigned *__restrict__ rlines, const unsigned long long *__restrict__ rbytes,
                                                                   const unsigned long long *__restrict__ tbase, unsigned char *lstatus,
                                                                   unsigned char *out, unsigned long long max_bytes, xrit_image_line *lines,
                                                                   unsigned long long max_lines)
{
    const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
    unsigned np, nf;
    if (!images_counts(fs, max_pieces_in, max_files_in, np, nf)) return;
    for (unsigned p = wave; p < np; p += n_waves) {
        const xrit_file_piece pc = pieces[p];
        const unsigned f = pc.file;
        if (f >= nf) continue;
        const ImageMark m = mark[f];
        if (!m.rice) continue;
        const xrit_file_record r = files[f];
        const unsigned j = p - (r.first_piece + r.n_pieces - m.n_lines);        // (unsigned: a piece in front of the lines is beyond them)
        if (j >= m.n_lines) continue;
        const unsigned long long *tb = tbase + (size_t)(f / IMAGES_TILE) * 2;
        const unsigned long long line = tb[0] + rlines[f] + j, off = tb[1] + rbytes[f] + (unsigned long long)j * m.padded;
        const unsigned n = r.bits_per_pixel, J = r.pixels_per_block, S = r.columns, length = image_line_bytes(r);
        const bool fits = off + m.padded <= max_bytes;
        unsigned char *dst = out + off;
        if (pc.offset > n_bytes || pc.length > n_bytes - pc.offset || pc.length > RICE_MAX_LINE) {
            if (fits)
                for (unsigned i = lane; i < length; i += 64) dst[i] = 0;
            if (lane == 0) lstatus[p] = 2;
        } else if (!fits)
            decode_line_wave<unsigned char, false>(bytes + pc.offset, pc.length, n, J, S, nullptr, lstatus + p, lane);
        else if (n <= 8)
            decode_line_wave(bytes + pc.offset, pc.length, n, J, S, dst, lstatus + p, lane);
        else
            decode_line_wave(bytes + pc.offset, pc.length, n, J, S, reinterpret_cast<unsigned short *>(dst), lstatus + p, lane);
        if (fits && lane < m.padded - length) dst[length + lane] = 0;
        if (lane == 0 && line < max_lines) {
            xrit_image_line o{};
            o.offset = off;
            o.length = length;
            o.row = pc.index_in_file - 1u;
            o.file = f;
            o.piece = p;
            o.samples = (uint16_t)S;
            o.bits = (uint8_t)n;
            o.status = lstatus[p];
            lines[line] = o;
        }
    }
}

// (d) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * WAVES) images_records_kernel(const xrit_file_record *__restrict__ files, unsigned long long max_pieces_in,
                                                                    unsigned long long max_files_in, const xrit_files_summary *__restrict__ fs,
                                                                    const ImageMark *__restrict__ mark, const unsigned *__restrict__ rlines,
                                                                    const unsigned long long *__restrict__ rbytes,
                                                                    const unsigned long long *__restrict__ tbase,
                                                                    const unsigned char *__restrict__ lstatus, unsigned *__restrict__ rfaults,
                                                                    xrit_image_key *__restrict__ keys, xrit_image_file *__restrict__ image_files)
{
    const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
    unsigned np, nf;
    if (!images_counts(fs, max_pieces_in, max_files_in, np, nf)) return;
    for (unsigned f = wave; f < nf; f += n_waves) {
        const ImageMark m = mark[f];
        const xrit_file_record r = files[f];
        unsigned faults = 0;
        if (m.rice) {
            const unsigned first = r.first_piece + r.n_pieces - m.n_lines;      // (mark: the record's pieces are all inside the call's)
            for (unsigned j = lane; j < m.n_lines; j += 64) faults += lstatus[first + j] != 0;
            faults = wave_sum(faults);
        }
        if (lane == 0) {
            rfaults[f] = faults;
            xrit_image_file o{};
            if (m.rice) {
                const unsigned long long *tb = tbase + (size_t)(f / IMAGES_TILE) * 2;
                o.offset = tb[1] + rbytes[f];
                o.length = (unsigned long long)m.n_lines * m.padded;
                o.first_line = (uint32_t)(tb[0] + rlines[f]);
                o.n_lines = m.n_lines;
                o.first_row = m.first_row;
                o.faults = faults;
                o.lines_total = m.base_lines + m.n_lines;
                o.faults_total = m.base_faults + faults;
                o.columns = r.columns;
                o.bits = r.bits_per_pixel;
                o.rice = 1;
            }
            image_files[f] = o;
            // the key's state is its last record's (records of one key are contiguous)
            const bool last = r.vcid < NVC && r.apid < 2048 && (f + 1 >= nf || files[f + 1].vcid != r.vcid || files[f + 1].apid != r.apid);
            if (last) keys[(unsigned)r.vcid * 2048u + r.apid] = image_next(r, m, faults);
        }
    }
}

__global__ void __launch_bounds__(256) images_finish_kernel(const xrit_files_summary *__restrict__ fs, unsigned long long max_pieces_in,
                                                            unsigned long long max_files_in, const unsigned *__restrict__ rfaults,
                                                            const unsigned long long *__restrict__ call, xrit_images_counters *__restrict__ counters,
                                                            xrit_images_summary *__restrict__ sum, unsigned long long max_lines,
                                                            unsigned long long max_bytes)
{
    __shared__ unsigned long long s_f[4];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    unsigned np, nf;
    const bool run = images_counts(fs, max_pieces_in, max_files_in, np, nf);
    unsigned long long faults = 0;
    for (unsigned f = tid; f < nf; f += 256u) faults += rfaults[f];
    faults = wave_sum(faults);
    if (lane == 0) s_f[tid >> 6] = faults;
    __syncthreads();
    if (tid != 0) return;
    xrit_images_counters t = *counters;
    xrit_images_summary o{};
    if (run) {
        o.lines = call[0];
        o.bytes = call[1];
        o.images = call[2];
        t.images_begun += call[3];
        t.images_completed += call[4];
        t.images_aborted += call[5];
        t.total_lines += call[0];
        t.total_faults += s_f[0] + s_f[1] + s_f[2] + s_f[3];
        t.total_bytes += call[1];
        *counters = t;
    }
    o.images_begun = t.images_begun;
    o.images_completed = t.images_completed;
    o.images_aborted = t.images_aborted;
    o.total_lines = t.total_lines;
    o.total_faults = t.total_faults;
    o.total_bytes = t.total_bytes;
    o.overflow = !run ? 2u : ((o.lines > max_lines || o.bytes > max_bytes) ? 1u : 0u);
    *sum = o;
}

size_t images_scratch_carve(void *base, size_t max_files_in, size_t max_pieces_in, ImagesScratch &sc)
{
    const size_t R = max_files_in ? max_files_in : 1, P = max_pieces_in ? max_pieces_in : 1, T = div_up(R, IMAGES_TILE);
    Carver c{static_cast<char *>(base)};
    sc.mark = c.take<ImageMark>(R, 16);
    sc.rbytes = c.take<unsigned long long>(R, 16);
    sc.tsum = c.take<unsigned long long>(T * IMAGES_TSUM, 16);
    sc.tbase = c.take<unsigned long long>(T * 2, 16);
    sc.call = c.take<unsigned long long>(IMAGES_TSUM, 16);
    sc.rlines = c.take<unsigned>(R, 16);
    sc.rfaults = c.take<unsigned>(R, 16);
    sc.lstatus = c.take<unsigned char>(P, 16);
    return c.used();
}

int launch_images(const unsigned char *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t max_pieces_in,
                  const xrit_file_record *files, size_t max_files_in, const xrit_files_summary *fsum, xrit_image_key *keys,
                  xrit_images_counters *counters, ImagesScratch &sc, unsigned char *out, size_t max_bytes, xrit_image_line *lines,
                  size_t max_lines, xrit_image_file *image_files, xrit_images_summary *summary, hipStream_t s)
{
    const unsigned long long bp = max_pieces_in, bf = max_files_in;
    const size_t R = max_files_in ? max_files_in : 1, P = max_pieces_in ? max_pieces_in : 1;
    // (the counts are on the device: grids no larger than fill the chip a few times over, striding)
    const unsigned g_mark = div_up(R, 256), g_tile = div_up(R, IMAGES_TILE), g_piece = div_up(P, WAVES), g_rec = div_up(R, WAVES);
    hipLaunchKernelGGL(images_mark_kernel, dim3(g_mark < 1024u ? g_mark : 1024u), dim3(256), 0, s, pieces, bp, files, bf, fsum, keys, sc.mark,
                       sc.rlines, sc.rbytes);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(images_tile_kernel, dim3(g_tile < 512u ? g_tile : 512u), dim3(IMAGES_TILE), 0, s, fsum, bp, bf, sc.mark, sc.rlines,
                       sc.rbytes, sc.tsum);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(images_total_kernel, dim3(1), dim3(64), 0, s, fsum, bp, bf, sc.tsum, sc.tbase, sc.call);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(images_decode_kernel, dim3(g_piece < 8192u ? g_piece : 8192u), dim3(64 * WAVES), 0, s, bytes,
                       (unsigned long long)n_bytes, pieces, bp, files, bf, fsum, sc.mark, sc.rlines, sc.rbytes, sc.tbase, sc.lstatus, out,
                       (unsigned long long)max_bytes, lines, (unsigned long long)max_lines);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(images_records_kernel, dim3(g_rec < 4096u ? g_rec : 4096u), dim3(64 * WAVES), 0, s, files, bp, bf, fsum, sc.mark,
                       sc.rlines, sc.rbytes, sc.tbase, sc.lstatus, sc.rfaults, keys, image_files);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(images_finish_kernel, dim3(1), dim3(256), 0, s, fsum, bp, bf, sc.rfaults, sc.call, counters, summary,
                       (unsigned long long)max_lines, (unsigned long long)max_bytes);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
