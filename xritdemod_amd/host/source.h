// source.h -- what main reads samples through: a reader callback (the capture file, or memory in the check program), in
// front of it the replay of what --acquire read ahead, behind it either fixed --block reads or the reference's FIFO
// chunking rule, and the pacing.  Plain C++: no library call, checked by `make host-program-check`.
//
// The FIFO rule (demodulator.cpp:38, :108-119, Parameters.h:57): the source delivers blocks of --fifo-block samples into a
// FIFO of FIFO_COMPLEX samples; the DSP loop looks at it after every --fifo-lag blocks and, once it holds FIFO_MIN_COMPLEX,
// takes EVERYTHING it holds as one chunk.  What does not fit the FIFO is lost and counted, with one message for the run.
// At the end of the input what is left below the threshold stays in the FIFO: the chunk is 0.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

constexpr size_t FIFO_COMPLEX = 1024 * 1024 / 2;      // FIFO_SIZE floats (Parameters.h:57)
constexpr size_t FIFO_MIN_COMPLEX = 64 * 1024 / 2;    // "Lets wait for more samples" (demodulator.cpp:113)

struct Source {
    std::function<size_t(void *, size_t)> reader;       // (destination, samples wanted) -> samples read, 0 at the end
    size_t bytes_per_sample = 8;
    bool paced = false;                                 // CFileFrontend.cpp:36-47: one block per block period
    double sample_rate = 2.5e6;
    std::chrono::steady_clock::time_point t_release = std::chrono::steady_clock::now();
    bool fifo = false;
    size_t fifo_block = 65535;
    int fifo_lag = 1;
    size_t fifo_fill = 0, fifo_overflowed = 0, fifo_calls = 0, fifo_min = ~(size_t)0, fifo_max = 0;
    bool fifo_eof = false;
    std::vector<unsigned char> ahead, blockbuf;
    size_t ahead_pos = 0;

    // --acquire: `want` samples read ahead of the run; read() hands them out again before the reader goes on
    size_t read_ahead(size_t want)
    {
        ahead.resize(want * bytes_per_sample);
        ahead.resize(reader(ahead.data(), want) * bytes_per_sample);
        return ahead.size() / bytes_per_sample;
    }
    size_t read(void *dst, size_t count)
    {
        if (ahead_pos >= ahead.size()) return reader(dst, count);
        size_t got = (ahead.size() - ahead_pos) / bytes_per_sample;
        got = got < count ? got : count;
        std::memcpy(dst, ahead.data() + ahead_pos, got * bytes_per_sample);
        ahead_pos += got * bytes_per_sample;
        if (got < count) got += reader(static_cast<unsigned char *>(dst) + got * bytes_per_sample, count - got);
        return got;
    }
    void pace(size_t n)
    {
        if (!paced) return;
        std::this_thread::sleep_until(t_release);
        t_release += std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>((double)n / sample_rate));
    }
    // the largest chunk next() can give: what `raw` has to hold
    size_t max_chunk(size_t block) const { return fifo ? FIFO_COMPLEX : block; }
    // the next chunk of the run into raw: the FIFO's, or one block; 0 at the end
    size_t next(unsigned char *raw, size_t block)
    {
        if (fifo) return fifo_chunk(raw);
        const size_t n = read(raw, block);
        if (n) pace(n);
        return n;
    }
    size_t fifo_chunk(unsigned char *raw)
    {
        blockbuf.resize(fifo_block * bytes_per_sample);
        // the source runs until the DSP loop looks again AND finds at least 64 Ki floats (:108-116)
        for (;;) {
            for (int b = 0; b < fifo_lag && !fifo_eof; ++b) {
                const size_t got = read(blockbuf.data(), fifo_block);
                if (got == 0) { fifo_eof = true; break; }
                pace(got);
                size_t take = got;
                if (fifo_fill + take > FIFO_COMPLEX) {
                    if (!fifo_overflowed) std::fprintf(stderr, "Input Samples Fifo is overflowing!\n");
                    fifo_overflowed += fifo_fill + take - FIFO_COMPLEX;
                    take = FIFO_COMPLEX - fifo_fill;
                }
                std::memcpy(raw + fifo_fill * bytes_per_sample, blockbuf.data(), take * bytes_per_sample);
                fifo_fill += take;
            }
            if (fifo_fill >= FIFO_MIN_COMPLEX || fifo_eof) break;
        }
        // (at the end of the file the reference's loop stops with what is left below the threshold still in the FIFO)
        if (fifo_fill < FIFO_MIN_COMPLEX) return 0;
        const size_t n = fifo_fill;
        fifo_fill = 0;
        ++fifo_calls;
        fifo_min = n < fifo_min ? n : fifo_min;
        fifo_max = n > fifo_max ? n : fifo_max;
        return n;
    }
    void report_fifo() const
    {
        std::fprintf(stderr, "fifo: %zu chunks of %zu .. %zu samples (source blocks of %zu, %d per look), %zu samples lost to overflow\n",
                     fifo_calls, fifo_calls ? fifo_min : 0, fifo_max, fifo_block, fifo_lag, fifo_overflowed);
    }
};
