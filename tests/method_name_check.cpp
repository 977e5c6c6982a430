// tests/method_name_check.cpp -- csrc/method_name.h on its own: the parser of eph_nbody_create's method string ("Name" or
// "Name<Double>") against every shape of input the boundary can be handed. Plain host C++ with a main of its own, so that it can
// also be built under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iephemeris_explorer_amd/csrc tests/method_name_check.cpp -o method_name_check
// Inputs live in exactly-sized heap blocks: a read past the terminator, or a write past `cap`, is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "method_name.h"

namespace {

int failures = 0;

// the input in a heap block of exactly strlen + 1 bytes, the output in one of exactly `cap`
void expect(const std::string &input, size_t cap, bool ok, const char *base, bool compensated) {
    char *in = static_cast<char *>(std::malloc(input.size() + 1));
    std::memcpy(in, input.c_str(), input.size() + 1);
    char *out = static_cast<char *>(std::malloc(cap ? cap : 1));
    if (cap) std::memset(out, 'x', cap);
    bool tag = true;
    const bool got = eph::parse_method_name(in, out, cap, &tag);
    const bool fine = got == ok && (!cap || std::memchr(out, '\0', cap)) && (!ok || (std::strcmp(out, base) == 0 && tag == compensated)) &&
                      (ok || !cap || out[0] == '\0');
    if (!fine) {
        std::printf("FAILED: \"%.40s\" (%zu bytes) cap %zu -> %d \"%.*s\" %d\n", in, input.size(), cap, (int)got, (int)(cap ? cap - 1 : 0), out, (int)tag);
        ++failures;
    }
    std::free(in);
    std::free(out);
}

}  // namespace

int main() {
    expect("QuinlanTremaine12", 64, true, "QuinlanTremaine12", false);
    expect("QuinlanTremaine12<Double>", 64, true, "QuinlanTremaine12", true);
    expect("Stormer13<Double>", 64, true, "Stormer13", true);
    expect("BlanesMoan14A<Double>", 64, true, "BlanesMoan14A", true);
    expect("NoSuchMethod<Double>", 64, true, "NoSuchMethod", true);          // (the table look-up refuses it, not the parser)
    expect("Ruth", 5, true, "Ruth", false);                                  // fits exactly
    // empty
    expect("", 64, false, "", false);
    expect("<Double>", 64, false, "", false);
    expect("<", 64, false, "", false);
    // other suffixes: case, white space, anything before, between or behind
    for (const char *bad : {"QuinlanTremaine12<Float>", "QuinlanTremaine12<double>", "QuinlanTremaine12<DOUBLE>", "QuinlanTremaine12<Double",
                            "QuinlanTremaine12<Double> ", "QuinlanTremaine12<Double>>", "QuinlanTremaine12<Double><Double>", "QuinlanTremaine12<>",
                            "QuinlanTremaine12<", "QuinlanTremaine12< Double>", "QuinlanTremaine12<Double >", "QuinlanTremaine12<Double>\n",
                            "QuinlanTremaine12<Doubl", "QuinlanTremaine12<D", "Quinlan<Double>Tremaine12"})
        expect(bad, 64, false, "", false);
    // unterminated-looking: the last byte before the terminator opens or half-closes a tag
    expect("Stormer13<Double", 64, false, "", false);
    expect("Stormer13<Doubl\xff", 64, false, "", false);
    // a blank is part of the base name (unknown to the tables later), not skipped
    expect("QuinlanTremaine12 <Double>", 64, true, "QuinlanTremaine12 ", true);
    expect(" Stormer13", 64, true, " Stormer13", false);
    // over-long: a base that does not fit `cap` with its terminator, with and without the tag; 1 MiB of name
    expect("Ruth", 4, false, "", false);
    expect("Ruth<Double>", 4, false, "", false);
    expect(std::string(63, 'A'), 64, true, std::string(63, 'A').c_str(), false);
    expect(std::string(64, 'A'), 64, false, "", false);
    expect(std::string(64, 'A') + "<Double>", 64, false, "", false);
    expect(std::string(1 << 20, 'B') + "<Double>", 64, false, "", false);
    expect(std::string(1 << 20, '<'), 64, false, "", false);
    expect("Ruth", 1, false, "", false);
    // no room, no arguments
    char base[8] = "xxxxxxx";
    bool tag = true;
    if (eph::parse_method_name("Ruth", base, 0, &tag) || eph::parse_method_name(nullptr, base, sizeof(base), &tag) ||
        eph::parse_method_name("Ruth", nullptr, 8, &tag) || eph::parse_method_name("Ruth", base, sizeof(base), nullptr)) {
        std::printf("FAILED: a missing argument was accepted\n");
        ++failures;
    }
    if (failures) return 1;
    std::printf("method_name: ok\n");
    return 0;
}
