// Library core of libbm2f: the per-thread error string, the ABI version and the tuning options (common.h,
// include/bm2f.h).  Every other file of the library depends on these.
#include "common.h"

#include <atomic>
#include <cstring>

namespace m2f {
std::string& last_error() {
  static thread_local std::string s;
  return s;
}
}  // namespace m2f

extern "C" const char* m2f_last_error(void) { return m2f::last_error().c_str(); }
extern "C" int m2f_abi_version(void) { return 1; }

namespace {
constexpr const char* kOptionNames[m2f::kOptCount] = {
#define M2F_OPTION_NAME(id, name) name,
    M2F_OPTIONS(M2F_OPTION_NAME)
#undef M2F_OPTION_NAME
};
std::atomic<int64_t> g_options[m2f::kOptCount] = {};
struct OptionInit {
  OptionInit() {
    for (auto& o : g_options) o.store(-1);
  }
} g_option_init;

int option_index(const char* name) {
  for (int i = 0; name && i < m2f::kOptCount; ++i)
    if (std::strcmp(name, kOptionNames[i]) == 0) return i;
  return -1;
}
}  // namespace

int64_t m2f::option_raw(Option o) { return g_options[o].load(std::memory_order_relaxed); }

extern "C" int m2f_set_option(const char* name, int64_t value) {
  const int i = option_index(name);
  if (i < 0) return m2f::fail(M2F_EINVAL, "m2f_set_option: unknown option '%s'", name ? name : "(null)");
  g_options[i].store(value < 0 ? -1 : value);
  return m2f::ok();
}

extern "C" int m2f_get_option(const char* name, int64_t* value) {
  const int i = option_index(name);
  if (i < 0 || !value) return m2f::fail(M2F_EINVAL, "m2f_get_option: unknown option '%s'", name ? name : "(null)");
  *value = g_options[i].load();
  return m2f::ok();
}
