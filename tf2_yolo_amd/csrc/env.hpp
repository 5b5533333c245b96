// Tuning knobs from the environment (YOLO_*). No HIP header: tests/test_host_cpu.py compiles this file with the host compiler.
#pragma once
#include <cstdlib>

namespace yolo {

// unset -> dflt, otherwise atoi / atoll of the text (so "" and "abc" give 0). Call sites cache: static const int v = env_int(...).
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}

}  // namespace yolo
