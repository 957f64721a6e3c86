// The table of process-wide options (gpet_options.h).  Host code only.
#include "gpet_options.h"

#include <cstdlib>
#include <cstring>
#include <mutex>

namespace gpet {

namespace {

const OptionDef kDefs[] = {
#define GPET_OPT_DEF(name, def, lo, hi, doc) {#name, def, lo, hi, doc},
    GPET_OPTIONS(GPET_OPT_DEF)
#undef GPET_OPT_DEF
};
constexpr int kCount = (int)(sizeof(kDefs) / sizeof(kDefs[0]));
static_assert(kCount <= kMaxOptions, "OptionSet holds every option");
int g_val[kMaxOptions];
std::once_flag g_once;
std::mutex g_mu;  // writers of the process-wide table and the snapshots of it
thread_local OptionSet* tl_set = nullptr;

int clampv(const OptionDef& d, int v) { return v < d.lo ? d.lo : (v > d.hi ? d.hi : v); }

void init_all() {
  for (int i = 0; i < kCount; ++i) {
    const OptionDef& d = kDefs[i];
    char env[64] = "GPET_";
    size_t n = strlen(env);
    for (const char* p = d.name; *p && n + 1 < sizeof env; ++p) env[n++] = (*p >= 'a' && *p <= 'z') ? (char)(*p - 32) : *p;
    env[n] = 0;
    const char* e = getenv(env);
    g_val[i] = e ? clampv(d, atoi(e)) : d.def;
  }
}

}  // namespace

int opt(Opt o) {
  std::call_once(g_once, init_all);
  return tl_set ? tl_set->v[(int)o] : g_val[(int)o];
}

int option_find(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < kCount; ++i)
    if (strcmp(kDefs[i].name, name) == 0) return i;
  return -1;
}

int option_set(OptionSet* s, int i, int value) {
  std::call_once(g_once, init_all);
  std::lock_guard<std::mutex> lk(g_mu);
  int* v = s ? s->v : g_val;
  const int prev = v[i];
  v[i] = clampv(kDefs[i], value);
  return prev;
}

int option_get(const OptionSet* s, int i) {
  std::call_once(g_once, init_all);
  std::lock_guard<std::mutex> lk(g_mu);
  return s ? s->v[i] : g_val[i];
}

void option_snapshot(OptionSet* out) {
  std::call_once(g_once, init_all);
  std::lock_guard<std::mutex> lk(g_mu);
  memcpy(out->v, g_val, sizeof out->v);
}

OptionScope::OptionScope(OptionSet* s) : prev(tl_set), active(s != nullptr) {
  if (active) tl_set = s;
}
OptionScope::~OptionScope() {
  if (active) tl_set = prev;
}

int option_count() { return kCount; }
const OptionDef& option_def(int i) { return kDefs[i]; }

}  // namespace gpet
