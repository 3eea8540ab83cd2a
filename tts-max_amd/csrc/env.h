// env.h — the one way to read a TTS_* switch.  atoi decides, so an empty or non-numeric value
// counts as 0.  Call sites keep the result in a function-local `static const`: a switch is
// read once per process.
#pragma once
#include <stdlib.h>

namespace tts {

// default on: only a value that reads as 0 turns the switch off
inline bool env_on(const char* name) {
  const char* v = getenv(name);
  return !(v && !atoi(v));
}
// default off: only a value that reads as non-zero turns the switch on
inline bool env_set(const char* name) {
  const char* v = getenv(name);
  return v && atoi(v);
}
inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
inline long long env_ll(const char* name, long long dflt) {
  const char* v = getenv(name);
  return v ? atoll(v) : dflt;
}

}  // namespace tts
