// env_switch.h — the one way a GGML_MI355X_* run-time switch is read (the table of all of them: INTEGRATION.md). A switch is read where it is
// used, once per process:   static const bool on = env_on(<name>);   — a function-local static, so nothing is parsed per node or per
// launch. (The three that configure a backend or the registry instead of a code path — GRAPHS, FUSION, VIRTUAL_DEVICES — are read at that init.)
#pragma once

#include <stdlib.h>

namespace mi355x {

// an integer; unset: dflt
static inline long long env_int(const char * name, long long dflt) { const char * e = getenv(name); return e ? atoll(e) : dflt; }
// on / off: a non-zero integer is on, anything else off; unset: dflt
static inline bool env_on(const char * name, bool dflt = true) { const char * e = getenv(name); return e ? atoi(e) != 0 : dflt; }
static inline double env_double(const char * name, double dflt) { const char * e = getenv(name); return e ? atof(e) : dflt; }
// set at all, whatever the value
static inline bool env_is_set(const char * name) { return getenv(name) != nullptr; }

} // namespace mi355x
