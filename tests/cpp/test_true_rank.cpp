// test_true_rank.cpp — the C++ mirror's rank-mode decoder (include/rlnc/full.hpp, Decoder::create with a mode): the
// SURVEY.md §0.5 vectors in both modes, clone, and one full decode.  Exit code 0 = all passed.
// Built and run by tests/test_gpu_true_rank.py on the GPU box.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rlnc/full.hpp"

using rlnc::RLNCError;
using rlnc::full::Decoder;
using rlnc::full::Encoder;

namespace {

int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

struct FixedVector {  // an "RNG" that draws one given coding vector
    const uint8_t *v;
    void fill_bytes(uint8_t *p, size_t n) { std::memcpy(p, v, n); }
};
struct SplitMix {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    void fill_bytes(uint8_t *p, size_t n) {
        for (size_t i = 0; i < n; ++i) p[i] = uint8_t(next());
    }
};

const uint8_t kFixture[4][6] = {{0, 0, 2, 0, 0, 3}, {0, 0, 0, 2, 2, 0}, {0, 0, 0, 0, 0, 2}, {0, 0, 0, 0, 0, 1}};

void test_fixture_and_full_decode() {
    SplitMix rng{42};
    std::vector<uint8_t> data(47);  // k = 6 pieces of 8 bytes
    rng.fill_bytes(data.data(), data.size());
    auto enc = Encoder::create(data, 6).unwrap();
    CHECK(enc.get_piece_byte_len() == 8);

    auto ref = Decoder::create(8, 6).unwrap();
    auto ref0 = Decoder::create(8, 6, RLNC_RANK_MODE_REFERENCE).unwrap();
    auto dec = Decoder::create(8, 6, RLNC_RANK_MODE_TRUE).unwrap();
    CHECK(ref.rank_mode() == 0 && ref0.rank_mode() == 0 && dec.rank_mode() == 1);
    CHECK(Decoder::create(8, 6).unwrap().rank_mode() == 0);  // the thread's context was left in mode 0
    for (int p = 0; p < 4; ++p) {
        FixedVector fv{kFixture[p]};
        const std::vector<uint8_t> piece = enc.code(fv);
        CHECK(ref.decode(piece).is_ok());  // the crate's answer: four useful pieces
        CHECK(ref0.decode(piece).is_ok());
        auto r = dec.decode(piece);
        if (p < 3)
            CHECK(r.is_ok());
        else
            CHECK(r.is_err() && r.error() == RLNCError::PieceNotUseful);
    }
    CHECK(ref.get_useful_piece_count() == 4 && ref0.get_useful_piece_count() == 4);
    CHECK(dec.get_useful_piece_count() == 3 && dec.get_received_piece_count() == 4 && dec.get_remaining_piece_count() == 3);
    CHECK(dec.get_decoded_data().error() == RLNCError::NotAllPiecesReceivedYet);

    Decoder twin = dec.clone();
    CHECK(twin.rank_mode() == 1 && twin.get_useful_piece_count() == 3);
    while (!dec.is_already_decoded()) (void)dec.decode(enc.code(rng));
    while (!twin.is_already_decoded()) (void)twin.decode(enc.code(rng));
    CHECK(dec.decode(enc.code(rng)).error() == RLNCError::ReceivedAllPieces);
    const auto a = dec.get_decoded_data().unwrap(), b = twin.get_decoded_data().unwrap();
    CHECK(a.size() == data.size() && std::memcmp(a.data(), data.data(), data.size()) == 0);
    CHECK(b.size() == data.size() && std::memcmp(b.data(), data.data(), data.size()) == 0);
}

}  // namespace

int main() {
    test_fixture_and_full_decode();
    std::printf("%s (%d failures)\n", g_fail ? "FAILED" : "all passed", g_fail);
    return g_fail ? 1 : 0;
}
