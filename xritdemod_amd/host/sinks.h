// sinks.h -- where the soft symbols go: the decoder's TCP socket or a file (Sink), SymbolManager's queue and its sender
// loop (--drop), the constellation tap (Diag), and the one host-side int8 quantiser.  Plain C++ and sockets: no library call.
#pragma once
#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// SymbolManager.cpp:43-46: soft symbol -> int8 (x127, clamp, C-cast truncation)
inline int8_t quantize_i8(float soft)
{
    float f = soft * 127;
    f = f > 127 ? 127 : f;
    f = f < -128 ? -128 : f;
    return (int8_t)(char)f;
}

// tcp://HOST:PORT -> host, port; false without a colon behind the scheme
inline bool split_host_port(const std::string &spec, std::string &host, std::string &port)
{
    const std::string hp = spec.substr(6);
    const size_t c = hp.rfind(':');
    if (c == std::string::npos) return false;
    host = hp.substr(0, c);
    port = hp.substr(c + 1);
    return true;
}

struct Sink {
    enum Kind { NONE, TCP, FILE_ } kind = NONE;
    int fd = -1;
    FILE *f = nullptr;
    std::string host;
    int port = 0;
    int tries = 30;
    int sndbuf = 0;
    size_t sent = 0;

    Sink() = default;
    Sink(const Sink &) = delete;
    Sink &operator=(const Sink &) = delete;
    ~Sink() { close_all(); }

    // tcp://HOST:PORT without a connection attempt (--drop: the sender loop connects)
    bool set_tcp(const std::string &spec)
    {
        std::string p;
        if (!split_host_port(spec, host, p)) { std::fprintf(stderr, "sink: tcp://HOST:PORT expected\n"); return false; }
        kind = TCP;
        port = std::atoi(p.c_str());
        return true;
    }
    bool open(const std::string &spec, int connect_tries)
    {
        tries = connect_tries;
        if (spec == "null") { kind = NONE; return true; }
        if (spec.rfind("file:", 0) == 0) {
            kind = FILE_;
            f = std::fopen(spec.c_str() + 5, "wb");
            if (!f) { std::perror("sink file"); return false; }
            return true;
        }
        if (spec.rfind("tcp://", 0) == 0) return set_tcp(spec) && connect_retry();
        std::fprintf(stderr, "sink: unknown spec %s\n", spec.c_str());
        return false;
    }
    bool connect_once()
    {
        addrinfo hints{}, *res = nullptr;
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_STREAM;
        if (getaddrinfo(host.c_str(), std::to_string(port).c_str(), &hints, &res) != 0 || !res) return false;
        fd = ::socket(res->ai_family, res->ai_socktype, res->ai_protocol);
        if (fd >= 0 && sndbuf > 0) (void)setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &sndbuf, sizeof sndbuf);
        bool ok = fd >= 0 && ::connect(fd, res->ai_addr, res->ai_addrlen) == 0;
        freeaddrinfo(res);
        if (!ok) {
            if (fd >= 0) ::close(fd);
            fd = -1;
            return false;
        }
        int one = 1;
        (void)setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        return true;
    }
    // SymbolManager.cpp:23-35: try, sleep one second, try again
    bool connect_retry()
    {
        for (int t = 0; t < tries; ++t) {
            std::fprintf(stderr, "Trying to connect to decoder at %s:%d\n", host.c_str(), port);
            if (connect_once()) return true;
            std::this_thread::sleep_for(std::chrono::seconds(1));
        }
        std::fprintf(stderr, "sink: no decoder at %s:%d\n", host.c_str(), port);
        return false;
    }
    void disconnected()
    {
        std::fprintf(stderr, "Disconnected from decoder.\n");
        ::close(fd);
        fd = -1;
    }
    bool send_all(const int8_t *p, size_t n)
    {
        sent += n;
        if (kind == NONE) return true;
        if (kind == FILE_) return std::fwrite(p, 1, n, f) == n;
        // pieces of at most SM_SOCKET_BUFFER_SIZE bytes, like SymbolManager::process
        while (n > 0) {
            size_t piece = n > 16384 ? 16384 : n;
            ssize_t w = ::send(fd, p, piece, MSG_NOSIGNAL);
            if (w <= 0) {
                disconnected();
                if (!connect_retry()) return false;
                continue;
            }
            p += w;
            n -= (size_t)w;
        }
        return true;
    }
    void close_all()
    {
        if (fd >= 0) ::close(fd);
        if (f) std::fclose(f);
        fd = -1;
        f = nullptr;
    }
};

// ---- SymbolManager's queue (--drop) ---------------------------------------------------------------------------
// SymbolManager::add / ::process (SymbolManager.cpp:37-52,78-106): the DSP thread queues soft symbols, the sender
// thread takes at most 16384 of them at a time, quantises and sends.  Two ways to lose symbols, both kept: add() drops
// its whole chunk when the queue already holds `cap` symbols, process() empties the queue while no decoder is connected.
struct SymbolQueue {
    std::deque<float> q;
    std::mutex m;
    size_t cap = 1024 * 1024;
    size_t dropped_full = 0, dropped_disconnected = 0, peak = 0;

    void add(const float *sym, size_t n)
    {
        std::lock_guard<std::mutex> g(m);
        if (q.size() >= cap) {
            std::fprintf(stderr, "SymbolManager Buffer is full!!! Dropping samples.\n");
            dropped_full += n;
            return;
        }
        q.insert(q.end(), sym, sym + n);
        if (q.size() > peak) peak = q.size();
    }
    size_t take(int8_t *out, size_t max)
    {
        std::lock_guard<std::mutex> g(m);
        const size_t n = q.size() < max ? q.size() : max;
        for (size_t i = 0; i < n; ++i) {
            out[i] = quantize_i8(q.front());
            q.pop_front();
        }
        return n;
    }
    void clear_disconnected()
    {
        std::lock_guard<std::mutex> g(m);
        dropped_disconnected += q.size();
        q.clear();
    }
    size_t size()
    {
        std::lock_guard<std::mutex> g(m);
        return q.size();
    }
    // decoder/src/Statistics.h:34: one byte, percent of the capacity (a chunk may overshoot the capacity: clamped)
    static unsigned usage(size_t fill, size_t cap)
    {
        const size_t pc = cap ? fill * 100 / cap : 0;
        return (unsigned)(pc > 255 ? 255 : pc);
    }
};

// the reference's symbolThread / process() loop (--drop): connect attempts happen HERE, next to the DSP, not before it.
// It ends when the DSP is done and the queue is empty, or when two attempts in a row fail after the DSP is done.
inline void run_sender(Sink &sink, SymbolQueue &queue, const std::atomic<bool> &dsp_done)
{
    std::vector<int8_t> buf(16384);
    bool connected = false;
    int failed = 0;
    for (;;) {
        if (!connected) {
            std::fprintf(stderr, "Trying to connect to decoder at %s:%d\n", sink.host.c_str(), sink.port);
            connected = sink.connect_once();
            if (!connected) {
                queue.clear_disconnected();          // SymbolManager.cpp:78-83
                if (dsp_done.load() && ++failed >= 2) return;
                std::this_thread::sleep_for(std::chrono::seconds(1));
                continue;
            }
        }
        const size_t n = queue.take(buf.data(), buf.size());
        if (n == 0) {
            if (dsp_done.load()) return;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
            continue;
        }
        size_t off = 0;
        while (off < n) {
            const ssize_t w = ::send(sink.fd, buf.data() + off, n - off, MSG_NOSIGNAL);
            if (w <= 0) {
                sink.disconnected();
                connected = false;
                break;                                 // the rest of this piece is lost, like the reference's
            }
            off += (size_t)w;
        }
        sink.sent += off;
    }
}

// ---- constellation tap (DiagManager) -----------------------------------------------------------------------
struct Diag {
    int fd = -1;
    sockaddr_in to{};
    std::deque<float> q;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now() - std::chrono::seconds(1);
    static constexpr size_t CAP = 1u << 16;            // the reference's buffer simply stops taking samples when full

    Diag() = default;
    Diag(const Diag &) = delete;
    Diag &operator=(const Diag &) = delete;
    ~Diag() { if (fd >= 0) ::close(fd); }

    bool open(const std::string &spec)
    {
        if (spec.rfind("udp://", 0) != 0) { std::fprintf(stderr, "diag: udp://HOST:PORT expected\n"); return false; }
        std::string host, port;
        if (!split_host_port(spec, host, port)) return false;
        addrinfo hints{}, *res = nullptr;
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_DGRAM;
        if (getaddrinfo(host.c_str(), port.c_str(), &hints, &res) != 0 || !res) return false;
        std::memcpy(&to, res->ai_addr, sizeof to);
        freeaddrinfo(res);
        fd = ::socket(AF_INET, SOCK_DGRAM, 0);
        if (fd < 0) return false;
        sockaddr_in from{};
        from.sin_family = AF_INET;
        from.sin_addr.s_addr = htonl(INADDR_ANY);
        from.sin_port = htons(9001);                   // DiagManager.cpp:30; not fatal if somebody else holds it
        (void)::bind(fd, reinterpret_cast<sockaddr *>(&from), sizeof from);
        return true;
    }
    // demodulator.cpp:161-163: (float *)symbols, min(symbols, 1024) FLOATS
    void add(const float *iq, size_t nsym)
    {
        size_t nf = nsym < 1024 ? nsym : 1024;
        if (q.size() + nf > CAP) return;
        q.insert(q.end(), iq, iq + nf);
    }
    // DiagManager.cpp:24-62: x128 (not the sink's x127), clamp, truncation; one datagram of 1024 bytes at most every 10 ms
    void pump()
    {
        const auto now = std::chrono::steady_clock::now();
        if (q.size() < 1024 || now - last < std::chrono::milliseconds(10)) return;
        char data[1024];
        for (int i = 0; i < 1024; ++i) {
            float v = q.front() * 128.f;
            q.pop_front();
            v = v > 127 ? 127 : v;
            v = v < -128 ? -128 : v;
            data[i] = static_cast<char>(v);
        }
        (void)::sendto(fd, data, sizeof data, 0, reinterpret_cast<const sockaddr *>(&to), sizeof to);
        last = now;
    }
};
