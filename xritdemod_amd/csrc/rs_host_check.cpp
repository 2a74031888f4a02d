// rs_host_check.cpp -- rs_solve (rs_core.h: Berlekamp-Massey, Chien, Forney) in a host program of its own, on a volume of
// input the device never sees: random error patterns of every weight 0 .. 48, patterns whose values are solved so that
// chosen syndromes vanish (zero discrepancies), and words next to another codeword.  The encoder here is its own LFSR
// from the generator roots.  Built and run by `make rs-host-check` with -fsanitize=address,undefined; prints counts and
// exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rs_core.h"

using namespace xrit;

namespace {

const RsTables tb = rs_make_tables();

unsigned mul(unsigned a, unsigned b) { return rs_mul(a, b, tb.exp, tb.log); }
unsigned inv(unsigned a) { return tb.exp[255 - tb.log[a]]; }
unsigned root_pow(int pos, int i)          // X^(FCR + i) of the symbol at byte pos (degree 254 - pos), X = beta^degree
{
    return tb.exp[((RS_PRIM * (RS_NN - 1 - pos)) % RS_NN * (RS_FCR + i)) % RS_NN];
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()                              // xorshift64*
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
unsigned rnd_below(unsigned n) { return rnd() % n; }
unsigned rnd_value() { return 1 + rnd_below(255); }

// g(x) = prod (x - alpha^(11 (112 + i))), gen[j] the coefficient of x^j
uint8_t gen[RS_NROOTS + 1];
void make_generator()
{
    std::memset(gen, 0, sizeof gen);
    gen[0] = 1;
    for (int i = 0; i < RS_NROOTS; ++i) {
        const unsigned r = tb.exp[(RS_PRIM * (RS_FCR + i)) % RS_NN];
        for (int j = i + 1; j > 0; --j) gen[j] = (uint8_t)(gen[j - 1] ^ mul(gen[j], r));
        gen[0] = (uint8_t)mul(gen[0], r);
    }
}

// systematic LFSR encoder, conventional basis: cw[0 .. 222] data (byte 0 the highest degree), cw[223 .. 254] parity
void encode(uint8_t *cw)
{
    uint8_t par[RS_NROOTS] = {};                                   // par[0] the highest-degree parity symbol
    for (int j = 0; j < RS_NN - RS_NROOTS; ++j) {
        const unsigned fb = cw[j] ^ par[0];
        for (int q = 0; q < RS_NROOTS - 1; ++q) par[q] = (uint8_t)(par[q + 1] ^ mul(fb, gen[RS_NROOTS - 1 - q]));
        par[RS_NROOTS - 1] = (uint8_t)mul(fb, gen[0]);
    }
    std::memcpy(cw + RS_NN - RS_NROOTS, par, RS_NROOTS);
}

// the caller owns S on the heap (exactly 32 bytes), so that an index outside it is the sanitizer's to find
bool syndromes(const uint8_t *cw, uint8_t *S)
{
    bool any = false;
    for (int i = 0; i < RS_NROOTS; ++i) {
        const unsigned la = (unsigned)((RS_PRIM * (RS_FCR + i)) % RS_NN);
        unsigned s = 0;
        for (int j = 0; j < RS_NN; ++j) s = (s ? tb.exp[tb.log[s] + la] : 0u) ^ cw[j];
        S[i] = (uint8_t)s;
        any |= s != 0;
    }
    return any;
}

// the same by linearity, for a word that is a codeword plus the sparse pattern err: S_i = sum err[j] X_j^(FCR + i)
bool syndromes_of_pattern(const uint8_t *err, uint8_t *S)
{
    bool any = false;
    std::memset(S, 0, RS_NROOTS);
    for (int j = 0; j < RS_NN; ++j) {
        if (!err[j]) continue;
        const unsigned lx = (unsigned)((RS_PRIM * (RS_NN - 1 - j)) % RS_NN), le = tb.log[err[j]];
        for (int i = 0; i < RS_NROOTS; ++i) S[i] ^= tb.exp[(le + lx * (unsigned)(RS_FCR + i)) % RS_NN];
    }
    for (int i = 0; i < RS_NROOTS; ++i) any |= S[i] != 0;
    return any;
}

// `count` distinct byte positions in pos[], drawn from [lo, hi)
void draw_positions(int *pos, int count, int lo = 0, int hi = RS_NN)
{
    bool used[RS_NN] = {};
    for (int e = 0; e < count;) {
        const int p = lo + (int)rnd_below((unsigned)(hi - lo));
        if (!used[p]) { used[p] = true; pos[e++] = p; }
    }
}

struct Tally { long decoded = 0, corrected = 0, refused = 0, other_codeword = 0; };

// What the device kernel does with a codeword (rs.hip): syndromes, rs_solve when any is non-zero, corrections in place.
// word = a codeword + err, so the syndromes are the pattern's; every 64th call computes them from the word as well.
// where / mag are exactly RS_T long and on the heap.  Returns rs_solve's count (0 for zero syndromes, -1 refused).
int decode(uint8_t *word, const uint8_t *err)
{
    static unsigned long calls = 0;
    std::vector<uint8_t> S(RS_NROOTS), mag(RS_T);
    std::vector<int> where(RS_T);
    const bool any = syndromes_of_pattern(err, S.data());
    if (calls++ % 64 == 0) {
        std::vector<uint8_t> full(RS_NROOTS);
        if (syndromes(word, full.data()) != any || std::memcmp(full.data(), S.data(), RS_NROOTS) != 0) return -3;
    }
    if (!any) return 0;
    const int n = rs_solve(S.data(), tb.exp, tb.log, where.data(), mag.data());
    if (n < -1 || n == 0 || n > RS_T) return -2;
    for (int e = 0; e < n; ++e) {
        if (where[e] < 0 || where[e] >= RS_NN || mag[e] == 0) return -2;
        word[where[e]] ^= mag[e];
    }
    return n;
}

#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);        \
            std::fprintf(stderr, __VA_ARGS__);                                      \
            std::fprintf(stderr, "\n");                                             \
            return 1;                                                               \
        }                                                                           \
    } while (0)

// sent + err must come back as `want` with `count` corrections
int expect(const uint8_t *sent, const uint8_t *err, const uint8_t *want, int count, const char *what, int a, int b)
{
    uint8_t word[RS_NN];
    for (int j = 0; j < RS_NN; ++j) word[j] = sent[j] ^ err[j];
    const int n = decode(word, err);
    CHECK(n == count, "%s (%d, %d): rs_solve returned %d, expected %d", what, a, b, n, count);
    CHECK(std::memcmp(word, want, RS_NN) == 0, "%s (%d, %d): the corrected word is not the expected codeword", what, a, b);
    return 0;
}

// values on pos[0 .. v) with S_i = 0 for the nz (1 or 2) indices in zero[]: the last v - nz values are drawn, the first
// nz solved (one division, or Cramer's rule on the 2 x 2 system); false when a solved value comes out zero
bool solve_zero_syndromes(const int *pos, int v, const int *zero, int nz, uint8_t *val)
{
    for (int l = nz; l < v; ++l) val[l] = (uint8_t)rnd_value();
    unsigned rhs[2] = {0, 0};
    for (int q = 0; q < nz; ++q)
        for (int l = nz; l < v; ++l) rhs[q] ^= mul(val[l], root_pow(pos[l], zero[q]));
    if (nz == 1) {
        val[0] = (uint8_t)mul(rhs[0], inv(root_pow(pos[0], zero[0])));
    } else {
        const unsigned a = root_pow(pos[0], zero[0]), b = root_pow(pos[1], zero[0]);
        const unsigned c = root_pow(pos[0], zero[1]), d = root_pow(pos[1], zero[1]);
        const unsigned det = mul(a, d) ^ mul(b, c);
        if (det == 0) return false;
        val[0] = (uint8_t)mul(mul(rhs[0], d) ^ mul(b, rhs[1]), inv(det));
        val[1] = (uint8_t)mul(mul(a, rhs[1]) ^ mul(rhs[0], c), inv(det));
    }
    for (int l = 0; l < nz; ++l)
        if (val[l] == 0) return false;
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    const long per_weight = argc > 1 ? std::atol(argv[1]) : 10000, per_heavy = argc > 2 ? std::atol(argv[2]) : 2000;
    make_generator();
    {   // the encoder makes codewords, and g(x) has 33 non-zero coefficients
        int weight = 0;
        for (int j = 0; j <= RS_NROOTS; ++j) weight += gen[j] != 0;
        CHECK(weight == 33 && gen[RS_NROOTS] == 1, "generator weight %d", weight);
        uint8_t one[RS_NN] = {};
        one[222] = 1;
        encode(one);
        for (int j = 0; j <= RS_NROOTS; ++j) CHECK(one[222 + j] == gen[RS_NROOTS - j], "encode(x^32) is not g(x) at %d", j);
    }
    uint8_t sent[RS_NN], err[RS_NN], want[RS_NN];
    std::vector<uint8_t> S(RS_NROOTS);
    int pos[RS_NN];
    Tally t;

    // ---- every weight 0 .. 16 on random positions and values: back to the sent word with that count ----
    for (int v = 0; v <= RS_T; ++v) {
        for (long it = 0; it < per_weight; ++it) {
            if (it % 64 == 0) {
                for (int j = 0; j < RS_NN - RS_NROOTS; ++j) sent[j] = (uint8_t)rnd();
                encode(sent);
                CHECK(!syndromes(sent, S.data()), "the encoder's word has non-zero syndromes");
            }
            std::memset(err, 0, sizeof err);
            // a quarter of the patterns hold the ends (bytes 0 and 254), a quarter lie in the parity alone
            const int kind = (int)(it & 3);
            if (kind == 1 && v >= 2) {
                draw_positions(pos, v - 2, 1, RS_NN - 1);
                pos[v - 2] = 0;
                pos[v - 1] = RS_NN - 1;
            } else if (kind == 2) {
                draw_positions(pos, v, RS_NN - RS_NROOTS, RS_NN);
            } else {
                draw_positions(pos, v);
            }
            for (int e = 0; e < v; ++e) err[pos[e]] = (uint8_t)rnd_value();
            if (expect(sent, err, sent, v, "random pattern of weight", v, (int)it)) return 1;
            ++t.decoded;
            ++t.corrected;
        }
    }
    {   // all-zero syndromes are the caller's case: rs_solve refuses them
        std::vector<uint8_t> zero(RS_NROOTS, 0), mag(RS_T);
        std::vector<int> where(RS_T);
        CHECK(rs_solve(zero.data(), tb.exp, tb.log, where.data(), mag.data()) == -1, "zero syndromes");
    }

    // ---- zero discrepancies: values solved so that S_0, S_0 and S_1, a middle S_i, or S_31 vanish ----
    long zero_cases = 0;
    const int zsets[][3] = {{1, 0, 0}, {2, 0, 1}, {1, 15, 0}, {1, 16, 0}, {1, 7, 0}, {1, 31, 0}, {2, 30, 31}, {2, 0, 31}};
    for (int v : {2, 3, 8, 16}) {
        for (const auto &z : zsets) {
            const int nz = z[0];
            if (nz >= v) continue;                                  // two vanishing syndromes need three errors
            for (int it = 0; it < 200;) {
                uint8_t val[RS_T];
                draw_positions(pos, v);
                if (!solve_zero_syndromes(pos, v, z + 1, nz, val)) continue;
                std::memset(err, 0, sizeof err);
                for (int e = 0; e < v; ++e) err[pos[e]] = val[e];
                syndromes(err, S.data());
                for (int q = 0; q < nz; ++q) CHECK(S[z[1 + q]] == 0, "constructed S_%d is not zero", z[1 + q]);
                if (expect(sent, err, sent, v, "zero syndrome pattern", v, z[1])) return 1;
                ++it;
                ++zero_cases;
            }
        }
    }

    // ---- another codeword's sphere: 33 - j symbols of scale * x^shift * g(x) ----
    long near_cases = 0;
    for (int j : {1, 8, 16, 17}) {
        for (int it = 0; it < 300; ++it) {
            const int shift = it < 3 ? (it == 0 ? 0 : it == 1 ? 222 : 111) : (int)rnd_below(223);
            const unsigned scale = rnd_value();
            uint8_t g[RS_NN] = {};
            for (int q = 0; q <= RS_NROOTS; ++q) g[RS_NN - 1 - shift - q] = (uint8_t)mul(scale, gen[q]);
            CHECK(!syndromes(g, S.data()), "scale * x^shift * g(x) is not a codeword");
            std::memcpy(err, g, RS_NN);
            draw_positions(pos, j, RS_NN - 1 - shift - RS_NROOTS, RS_NN - shift);
            for (int e = 0; e < j; ++e) err[pos[e]] = 0;            // drop j of its 33 symbols
            for (int q = 0; q < RS_NN; ++q) want[q] = j <= RS_T ? sent[q] ^ g[q] : sent[q];
            if (expect(sent, err, want, j <= RS_T ? j : 33 - j, "near-codeword pattern", j, shift)) return 1;
            ++near_cases;
        }
    }

    // ---- weights 17 .. 48: refused, or a codeword ----
    for (int v = RS_T + 1; v <= 48; ++v) {
        for (long it = 0; it < per_heavy; ++it) {
            uint8_t word[RS_NN];
            draw_positions(pos, v);
            std::memset(err, 0, sizeof err);
            for (int e = 0; e < v; ++e) err[pos[e]] = (uint8_t)rnd_value();
            for (int j = 0; j < RS_NN; ++j) word[j] = sent[j] ^ err[j];
            const int n = decode(word, err);
            CHECK(n == -1 || (n >= 1 && n <= RS_T), "weight %d: rs_solve returned %d", v, n);
            if (n >= 0) {
                CHECK(!syndromes(word, S.data()), "weight %d: %d corrections do not give a codeword", v, n);
                ++t.other_codeword;
            } else {
                ++t.refused;
            }
            ++t.decoded;
        }
    }
    std::printf("rs host check ok: %ld words decoded, %ld corrected to the sent word (weights 0 .. 16), %ld with chosen zero "
                "syndromes, %ld next to another codeword, weights 17 .. 48: %ld refused, %ld taken to a codeword\n",
                t.decoded + zero_cases + near_cases, t.corrected, zero_cases, near_cases, t.refused, t.other_codeword);
    return 0;
}
