// method_name.h -- the method string of eph_nbody_create: "Name" or "Name<Double>" (Rust's `M<_>` over
// Vec<Double<DVec3>>, ephemeris/tests/solar_system_convergence.rs:112-199). Plain C++, no device code: the parser is also
// built on its own under the host sanitizers (tests/method_name_check.cpp).
#pragma once
#include <cstddef>
#include <cstring>

namespace eph {

// -> the base name in base[0, cap) (always terminated when cap > 0) and *compensated. false, with base empty, for a NULL
// argument, an empty base name, a base name that does not fit, or any suffix other than the exact, case-sensitive
// "<Double>" (no white space anywhere: a name with a blank is simply an unknown name to the caller's table look-up).
inline bool parse_method_name(const char *method, char *base, size_t cap, bool *compensated) {
    static const char kTag[] = "<Double>";
    if (base && cap) base[0] = '\0';
    if (!method || !base || !cap || !compensated) return false;
    *compensated = false;
    const char *lt = std::strchr(method, '<');
    const size_t len = lt ? (size_t)(lt - method) : std::strlen(method);
    if (len == 0 || len >= cap) return false;
    if (lt && std::strcmp(lt, kTag) != 0) return false;
    std::memcpy(base, method, len);
    base[len] = '\0';
    *compensated = lt != nullptr;
    return true;
}

}  // namespace eph
