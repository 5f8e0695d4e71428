// env.hpp — the three ways the library reads an environment knob.  Each reads the environment anew:
// a site that caches its knob keeps the result in a `static const` of its own, a site that is read
// per executor or per call calls these directly.
#pragma once
#include <cstdlib>

namespace phx {

// on unless set to "0..."
inline bool env_on(const char* name) {
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}

// off unless set to "1..."
inline bool env_flag(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '1';
}

// an integer, `dflt` when unset
inline long env_long(const char* name, long dflt) {
  const char* e = std::getenv(name);
  return e ? std::atol(e) : dflt;
}

}  // namespace phx
