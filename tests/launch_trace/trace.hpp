// Shared by stubs.hip and driver.cpp: the trace sink, the names of the fake addresses and the answers of the stubbed predicates.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

namespace lt {

// what the stubbed predicates answer: the driver sets them per case
struct Answers {
  size_t fused_lds_bytes = 0;
  bool h_chain_built = false;
  bool w_gsplit = false;
  int tail_nbk = 0;
};
inline Answers g_answers;

// ---- fake addresses: every pointer of the state is the base of a region of REGION bytes that nothing dereferences -------------
constexpr uintptr_t REGION = 0x1000000, FIRST = 0x10000000;
inline std::vector<std::string> g_regions;
inline void* fake(const char* name) {
  g_regions.push_back(name);
  return reinterpret_cast<void*>(FIRST + (g_regions.size() - 1) * REGION);
}
inline char* g_ev_base = nullptr;   // the region of the stubbed HIP events (driver.cpp registers it)
// "name+offset" of a fake address, "null", or "host" for anything else (a local of the code under test)
inline std::string pname(const void* p) {
  if (!p) return "null";
  const uintptr_t v = reinterpret_cast<uintptr_t>(p);
  if (v < FIRST || (v - FIRST) / REGION >= g_regions.size()) return "host";
  char off[32];
  snprintf(off, sizeof(off), "+%zu", (size_t)((v - FIRST) % REGION));
  return g_regions[(v - FIRST) / REGION] + ((v - FIRST) % REGION ? off : "");
}

// ---- the trace of one case: lines, collected so that a case can be shown or only summarised ------------------------------------
inline std::vector<std::string> g_lines;
inline std::string fmt(const char* f, ...) {
  char buf[4096];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}
inline void line(const std::string& s) { g_lines.push_back(s); }

// argument structs are long and repeat: the first time a value is seen it is written out as "def H3 = (...)", later as "H3".
// The table is reset per configuration (driver.cpp), so a difference does not renumber the rest of the file.
inline std::map<std::string, std::string> g_defs;
inline std::map<char, int> g_def_count;
inline std::string intern(char kind, const std::string& text) {
  auto it = g_defs.find(kind + text);
  if (it != g_defs.end()) return it->second;
  const std::string id = fmt("%c%d", kind, ++g_def_count[kind]);
  g_defs[kind + text] = id;
  line("def " + id + " = (" + text + ")");
  return id;
}
inline void reset_defs() {
  g_defs.clear();
  g_def_count.clear();
}

// one argument list: a.p(ptr).i(int).f(float) ... .str()
struct Args {
  std::string s;
  Args& add(const std::string& v) {
    if (!s.empty()) s += ",";
    s += v;
    return *this;
  }
  Args& p(const void* v) { return add(pname(v)); }
  Args& i(long long v) { return add(fmt("%lld", v)); }
  Args& u(unsigned long long v) { return add(fmt("%llu", v)); }
  Args& f(double v) { return add(fmt("%.9g", v)); }
  Args& t(const std::string& v) { return add(v); }
};
inline void call(const char* name, const Args& a) { line(std::string(name) + "(" + a.s + ")"); }

}  // namespace lt
