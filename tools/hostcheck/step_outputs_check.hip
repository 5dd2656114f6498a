// Host-only check of csrc/rec_state.h: the arena and mirror arithmetic (Carve, StepOutputs) and the engine's pure host checks (the mode
// exclusion table, slot lists, fans, the prompt store's ranges): no GPU, no HIP call. Meant to run under the host sanitizers, which see
// every byte StepOutputs::wait copies out of a mirror that is exactly host_bytes() long:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined \
//         tools/hostcheck/step_outputs_check.hip -o /tmp/step_outputs_check && /tmp/step_outputs_check
//
// The expected offsets and verdicts are written out by hand below.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "../../surya_amd/csrc/rec_state.h"

using sa::Carve;
using sa::StepOutputs;

static int failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// A set over fake device arrays (never dereferenced): `cells` bytes per cell and field.
static StepOutputs make(size_t slots, std::vector<size_t> cells) {
    StepOutputs o;
    o.slots = slots;
    for (size_t k = 0; k < cells.size(); ++k) o.add(reinterpret_cast<const void*>((k + 1) << 32), cells[k]);
    return o;
}

static void check_offsets(size_t S) {
    const size_t full = (size_t)SA_MAX_STEPS * S;
    for (int ring = 0; ring < 2; ++ring) {
        const int step = StepOutputs::ring_step(ring);
        CHECK(step == ring * SA_MAX_STEPS / 2);
        const size_t off = (size_t)ring * (SA_MAX_STEPS / 2) * S;
        for (int n = 0; n <= SA_MAX_STEPS / 2; ++n) {
            const size_t nt = (size_t)n * S;
            const StepOutputs base = make(S, {4, 4, 24});                  // token, score, box
            CHECK(base.host_bytes() == full * 32);
            CHECK(base.span(0, step, n).host == off * 4 && base.span(0, step, n).dev == off * 4 && base.span(0, step, n).bytes == nt * 4);
            CHECK(base.span(1, step, n).host == full * 4 + off * 4 && base.span(1, step, n).dev == off * 4);
            CHECK(base.span(2, step, n).host == full * 8 + off * 24 && base.span(2, step, n).dev == off * 24 && base.span(2, step, n).bytes == nt * 24);
            const size_t A = SA_MAX_ALTERNATIVES;
            const StepOutputs alts = make(S, {A * 4, A * 4});              // ids, probabilities
            CHECK(alts.host_bytes() == full * A * 8);
            CHECK(alts.span(0, step, n).host == off * A * 4 && alts.span(0, step, n).dev == off * A * 4 && alts.span(0, step, n).bytes == nt * A * 4);
            CHECK(alts.span(1, step, n).host == (full + off) * A * 4 && alts.span(1, step, n).dev == off * A * 4);
            const StepOutputs forced = make(S, {4, 4, 4});
            CHECK(forced.host_bytes() == full * 12);
            for (int k = 0; k < 3; ++k) CHECK(forced.span(k, step, n).host == ((size_t)k * full + off) * 4 && forced.span(k, step, n).dev == off * 4);
            const StepOutputs beam = make(S, {4, 4, 4, 4, 4});
            CHECK(beam.host_bytes() == full * 20);
            for (int k = 0; k < 5; ++k) CHECK(beam.span(k, step, n).host == ((size_t)k * full + off) * 4 && beam.span(k, step, n).bytes == nt * 4);
        }
    }
}

// wait() out of a mirror of exactly host_bytes() into destinations of exactly the bytes asked for: byte (field, step, slot, b) of the mirror
// carries a value that names it, so a wrong factor shows as a wrong value and a long copy as a sanitizer report.
static void check_wait(size_t S, std::vector<size_t> cells) {
    StepOutputs o = make(S, cells);
    std::vector<unsigned char> mirror(o.host_bytes());
    o.host = reinterpret_cast<char*>(mirror.data());
    auto tag = [&](int k, size_t step, size_t slot, size_t b) { return (unsigned char)(k * 131 + step * 31 + slot * 7 + b); };
    size_t at = 0;
    for (int k = 0; k < o.n; ++k)
        for (size_t step = 0; step < SA_MAX_STEPS; ++step)
            for (size_t slot = 0; slot < S; ++slot)
                for (size_t b = 0; b < cells[k]; ++b) mirror[at++] = tag(k, step, slot, b);
    CHECK(at == mirror.size());
    for (int ring = 0; ring < 2; ++ring)
        for (int n : {0, 1, 3, SA_MAX_STEPS / 2}) {
            std::vector<std::unique_ptr<unsigned char[]>> dst;          // (new[] of 0 bytes is still a pointer memcpy may be given)
            std::vector<void*> ptr;
            for (int k = 0; k < o.n; ++k) dst.emplace_back(new unsigned char[(size_t)n * S * cells[k]]);
            for (auto& d : dst) ptr.push_back(d.get());
            o.wait(ring, n, ptr.data());
            for (int k = 0; k < o.n; ++k) {
                size_t i = 0;
                for (size_t step = 0; step < (size_t)n; ++step)
                    for (size_t slot = 0; slot < S; ++slot)
                        for (size_t b = 0; b < cells[k]; ++b) CHECK(dst[k][i++] == tag(k, step + ring * SA_MAX_STEPS / 2, slot, b));
            }
        }
}

static void check_carve() {
    Carve cv;
    CHECK(cv.take(1) == 0 && cv.off == 256);
    CHECK(cv.take(256) == 256 && cv.off == 512);
    CHECK(cv.take(0) == 512 && cv.off == 512);                              // an empty block takes no room and shares its offset
    CHECK(cv.take(257) == 512 && cv.off == 1024);
    // the alternatives arena laid out by hand: aligned sizes summed up
    const size_t S = 24, vocab = 65792, A = SA_MAX_ALTERNATIVES, outs = (size_t)SA_MAX_STEPS * S * A;
    const size_t part_bytes = sa::align_up(S * ((vocab + 63) / 64) * A * 8), bt_bytes = sa::align_up(S * 8), out_b = sa::align_up(outs * 4);
    Carve c2;
    CHECK(c2.take(S * ((vocab + 63) / 64) * A * 8) == 0);
    CHECK(c2.take(S * 8) == part_bytes);
    CHECK(c2.take(outs * 4) == part_bytes + bt_bytes);
    CHECK(c2.take(outs * 4) == part_bytes + bt_bytes + out_b);
    CHECK(c2.off == part_bytes + bt_bytes + 2 * out_b);
}

// The exclusion table: row m, column p = "m may not be switched on while p is on", in the order of sa::Mode (masks, alternatives, forced,
// beam, fp8 KV, MXFP8, patterns, lexicon, boost). The 14 pairs of modes_excluded written out in both directions: 28 ones.
static void check_exclusions() {
    static const char* expect[sa::MODES] = {"001000000", "001000001", "110100111", "001011111", "000100000",
                                            "000100000", "001100001", "001100001", "011100110"};
    int ones = 0;
    for (int m = 0; m < sa::MODES; ++m) {
        const bool none[sa::MODES] = {};
        CHECK(!sa::modes_excluded(m, none));
        for (int p = 0; p < sa::MODES; ++p) {
            bool on[sa::MODES] = {};
            on[p] = true;
            CHECK(sa::modes_excluded(m, on) == (expect[m][p] == '1'));
            CHECK(expect[m][p] == expect[p][m]);
            ones += expect[m][p] == '1';
        }
    }
    CHECK(ones == 28);
    bool all[sa::MODES];
    for (bool& b : all) b = true;
    for (int m = 0; m < sa::MODES; ++m) CHECK(sa::modes_excluded(m, all));      // every mode has a partner
}

static void check_store_free() {
    std::map<int, int> live;
    CHECK(sa::store_free(live, 0, 1) && sa::store_free(live, 7, 100));         // an empty table
    live[10] = 5;                                                            // rows 10..14
    CHECK(sa::store_free(live, 5, 5));                                       // touches it from below
    CHECK(sa::store_free(live, 15, 3));                                      // ... from above
    CHECK(!sa::store_free(live, 6, 5));                                      // one row too far: row 10
    CHECK(!sa::store_free(live, 14, 3));                                     // starts on its last row
    CHECK(!sa::store_free(live, 11, 2) && !sa::store_free(live, 10, 5));      // inside it, and the entry itself
    CHECK(!sa::store_free(live, 8, 10));                                     // around it
    live[20] = 5;                                                            // rows 20..24
    CHECK(sa::store_free(live, 15, 5));                                      // touches both neighbours
    CHECK(!sa::store_free(live, 15, 6) && !sa::store_free(live, 14, 6));
    CHECK(sa::store_free(live, 0, 10) && sa::store_free(live, 25, 1));
}

static void check_slot_lists() {
    auto yes = [](int) { return true; };
    const int32_t ok[] = {0, 3}, high[] = {0, 4}, low[] = {-1}, twice[] = {1, 2, 1}, three[] = {0, 1, 2};
    CHECK(sa::check_slots(ok, 2, 4, yes) == SA_OK);
    CHECK(sa::check_slots(ok, 0, 4, yes) == SA_OK);
    CHECK(sa::check_slots(high, 2, 4, yes) == SA_ERR_ARG && sa::check_slots(high, 2, 5, yes) == SA_OK);      // out of range
    CHECK(sa::check_slots(low, 1, 4, yes) == SA_ERR_ARG);
    CHECK(sa::check_slots(twice, 3, 4, yes) == SA_ERR_ARG && sa::check_slots(twice, 2, 4, yes) == SA_OK);    // a repeated slot
    CHECK(sa::check_slots(three, 3, 4, [](int i) { return i != 2; }) == SA_ERR_ARG);                          // the predicate fails on the last entry
    CHECK(sa::check_slots(three, 2, 4, [](int i) { return i != 2; }) == SA_OK);
}

static void check_fan_lists() {
    auto yes = [](int, int) { return true; };
    const int32_t off[] = {0, 2, 3}, slots[] = {0, 1, 3};
    std::vector<std::pair<int, int>> seen;
    CHECK(sa::check_fans(off, slots, 2, 4, [&](int i, int j) { seen.emplace_back(i, j); return true; }) == SA_OK);
    CHECK((seen == std::vector<std::pair<int, int>>{{0, 0}, {0, 1}, {1, 2}}));                               // (fan, entry) as the predicate gets them
    CHECK(sa::check_fans(off, slots, 2, 4, [](int i, int) { return i == 0; }) == SA_ERR_ARG);
    const int32_t off1[] = {1, 2}, s1[] = {0, 1};
    CHECK(sa::check_fans(off1, s1, 1, 4, yes) == SA_ERR_ARG);                                                 // a non-zero first offset
    const int32_t empty[] = {0, 0, 1}, back[] = {0, 2, 1};
    CHECK(sa::check_fans(empty, slots, 2, 4, yes) == SA_ERR_ARG && sa::check_fans(back, slots, 2, 4, yes) == SA_ERR_ARG);      // an empty fan
    const int32_t many[] = {0, 3, 5}, s5[] = {0, 1, 2, 3, 0};
    CHECK(sa::check_fans(many, s5, 2, 4, yes) == SA_ERR_ARG);                                                 // five slots on a handle of four
    const int32_t full[] = {0, 3, 4}, rep[] = {0, 1, 2, 1};
    CHECK(sa::check_fans(full, s5, 2, 4, yes) == SA_OK && sa::check_fans(full, rep, 2, 4, yes) == SA_ERR_ARG);      // exactly max_slots; a slot in two fans
}

static void check_keep_ranges() {
    const int32_t seq[] = {0, 3, 8};                                         // two prompts of 3 and 5 rows
    const std::map<int, int> base = {{4, 4}};                                // rows 4..7 of a store of 16
    auto run = [&](int32_t a, int32_t b, int cap, std::map<int, int>* out) {
        const int32_t keep[] = {a, b};
        std::map<int, int> live = base;
        const int rc = sa::check_keep(live, keep, seq, 2, cap);
        if (out) *out = live;
        return rc;
    };
    std::map<int, int> live;
    CHECK(run(-1, -1, 16, &live) == SA_OK && live == base);
    CHECK(run(0, 8, 16, &live) == SA_OK && (live == std::map<int, int>{{0, 3}, {4, 4}, {8, 5}}));
    CHECK(run(1, 11, 16, &live) == SA_OK && live.size() == 3);               // touches the entry from below; ends on the store's last row
    CHECK(run(2, -1, 16, nullptr) == SA_ERR_ARG);                            // rows 2..4 reach into the entry
    CHECK(run(0, 12, 16, nullptr) == SA_ERR_ARG);                            // rows 12..16 of 16
    CHECK(run(8, 10, 16, nullptr) == SA_ERR_ARG);                            // the call's own two ranges overlap
    CHECK(run(-2, -1, 16, nullptr) == SA_ERR_ARG);
    CHECK(run(-1, 0, 4, nullptr) == SA_ERR_ARG);                             // five rows into a store of four
    CHECK(run(0, -1, 0, nullptr) == SA_ERR_ARG);                             // no store at all
}

int main() {
    for (size_t S : {1, 3, 24, 256, 1024}) check_offsets(S);
    for (size_t S : {1, 5, 24}) {
        check_wait(S, {4, 4, 24});
        check_wait(S, {16, 16});
        check_wait(S, {4, 4, 4});
        check_wait(S, {4, 4, 4, 4, 4});
    }
    check_carve();
    check_exclusions();
    check_store_free();
    check_slot_lists();
    check_fan_lists();
    check_keep_ranges();
    std::printf(failures ? "step_outputs_check: %d FAILED\n" : "step_outputs_check: ok\n", failures);
    return failures ? 1 : 0;
}


