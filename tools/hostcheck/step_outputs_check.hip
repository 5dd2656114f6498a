// Host-only check of the arena and mirror arithmetic of csrc/rec_engine.h (Carve, StepOutputs): no GPU, no HIP call. Meant to run under
// the host sanitizers, which see every byte StepOutputs::wait copies out of a mirror that is exactly host_bytes() long:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined \
//         tools/hostcheck/step_outputs_check.hip -o /tmp/step_outputs_check && /tmp/step_outputs_check
//
// The expected offsets are written out by hand below, per set and field.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../surya_amd/csrc/rec_engine.h"

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

int main() {
    for (size_t S : {1, 3, 24, 256, 1024}) check_offsets(S);
    for (size_t S : {1, 5, 24}) {
        check_wait(S, {4, 4, 24});
        check_wait(S, {16, 16});
        check_wait(S, {4, 4, 4});
        check_wait(S, {4, 4, 4, 4, 4});
    }
    check_carve();
    std::printf(failures ? "step_outputs_check: %d FAILED\n" : "step_outputs_check: ok\n", failures);
    return failures ? 1 : 0;
}
