// Error text, ABI version and the knob table (knobs.h) of libfod_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/fod.h"
#include "knobs.h"

static thread_local char g_err[512] = "";

void fod_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" size_t fod_last_error(char* buf, size_t cap) {
  const size_t n = strlen(g_err);
  if (buf && cap) {
    const size_t c = n < cap - 1 ? n : cap - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return n;
}

extern "C" int fod_abi_version(void) { return FOD_ABI_VERSION; }

extern "C" size_t fod_workspace_bytes(int kind) {
  switch (kind) {
    case FOD_WS_NT_SPLIT: return (size_t)FOD_NT_SPLIT_WS_FLOATS * sizeof(float);
    case FOD_WS_NT_SPLIT_TICKETS: return (size_t)FOD_NT_SPLIT_TICKETS * sizeof(unsigned);
    case FOD_WS_TN_PARTIALS: return FOD_TN_WS_BYTES;
    case FOD_WS_ATTN_SPLIT_PER_TILE: return (size_t)FOD_ATTN_SPLIT_WS_FLOATS_PER_TILE * sizeof(float);
    case FOD_WS_DET: return FOD_DET_WS_BYTES;
    case FOD_WS_TN_MULTI_DET: return FOD_TN_MULTI_DET_WS_BYTES;
    default: return 0;
  }
}

// ---- knobs.h: the table, its names, and the only getenv of the library
namespace {
struct KnobName {
  const char* name;
  int Knobs::*i;       // an int knob, or
  double Knobs::*d;    // a double one
};
const KnobName KNOB_NAMES[] = {
    {"FOD_NT_SMALL", &Knobs::nt_small, nullptr},
    {"FOD_NT_NARROW", &Knobs::nt_narrow, nullptr},
    {"FOD_NT_SPLITK", &Knobs::nt_splitk, nullptr},
    {"FOD_NT_BIG", &Knobs::nt_big, nullptr},
    {"FOD_NT_BIG256", &Knobs::nt_big256, nullptr},
    {"FOD_NT_BIG_ILV", &Knobs::nt_big_ilv, nullptr},
    {"FOD_NT_BIG256_MINK", &Knobs::nt_big256_mink, nullptr},
    {"FOD_NT_BIG_MINK", &Knobs::nt_big_mink, nullptr},
    {"FOD_NT_BIG_MINN", &Knobs::nt_big_minn, nullptr},
    {"FOD_TN_SMALL", &Knobs::tn_small, nullptr},
    {"FOD_TN_BIG", &Knobs::tn_big, nullptr},
    {"FOD_TN_BIG_DENSE", &Knobs::tn_big_dense, nullptr},
    {"FOD_TN_BIG256", &Knobs::tn_big256, nullptr},
    {"FOD_TN_BIG_MIN", nullptr, &Knobs::tn_big_min},
    {"FOD_TN_BIG_SPLITS", &Knobs::tn_big_splits, nullptr},
    {"FOD_TN_WS", &Knobs::tn_ws, nullptr},
    {"FOD_TN_XCD", &Knobs::tn_xcd, nullptr},
    {"FOD_TN_ROWS", &Knobs::tn_rows, nullptr},
    {"FOD_ATTN_LDS", &Knobs::attn_lds, nullptr},
    {"FOD_ATTN_PF", &Knobs::attn_pf, nullptr},
    {"FOD_FP8_STAGE", &Knobs::fp8_stage, nullptr},
    {"FOD_LN_BWD_GROUPS", &Knobs::ln_bwd_groups, nullptr},
    {"FOD_BNK_VERSION", &Knobs::bnk_version, nullptr},
};

// text -> field; "auto" only where the default is AUTO.  false: not a value of this knob
bool knob_parse(const KnobName& k, const char* text, Knobs& t) {
  char* end = nullptr;
  if (k.d) {
    const double v = strtod(text, &end);
    if (end == text || *end) return false;
    t.*k.d = v;
    return true;
  }
  if (Knobs{}.*k.i == Knobs::AUTO && !strcmp(text, "auto")) {
    t.*k.i = Knobs::AUTO;
    return true;
  }
  const long v = strtol(text, &end, 10);
  if (end == text || *end || v < 0 || v > 0x7FFFFFFF) return false;
  t.*k.i = (int)v;
  return true;
}

std::mutex g_knob_mutex;
Knobs& knob_table() {                  // call with g_knob_mutex held
  static Knobs table = [] {
    Knobs t;
    for (const KnobName& k : KNOB_NAMES)
      if (const char* text = getenv(k.name)) knob_parse(k, text, t);      // (a value that does not parse: the default)
    return t;
  }();
  return table;
}
const KnobName* knob_find(const char* name) {
  for (const KnobName& k : KNOB_NAMES)
    if (name && !strcmp(name, k.name)) return &k;
  fod_set_error("knob: unknown name %s", name ? name : "(null)");
  return nullptr;
}
}  // namespace

Knobs fod_knobs() {
  std::lock_guard<std::mutex> lock(g_knob_mutex);
  return knob_table();
}

extern "C" int fod_knob_set(const char* name, const char* value) {
  const KnobName* k = knob_find(name);
  if (!k) return FOD_ERR_ARG;
  std::lock_guard<std::mutex> lock(g_knob_mutex);
  Knobs& t = knob_table();
  if (!value) {
    const Knobs def;
    if (k->d) t.*k->d = def.*k->d;
    else t.*k->i = def.*k->i;
  } else if (!knob_parse(*k, value, t)) {
    fod_set_error("knob: %s cannot be '%s'", name, value);
    return FOD_ERR_ARG;
  }
  return FOD_OK;
}

extern "C" int fod_knob_get(const char* name, char* out, size_t out_bytes) {
  const KnobName* k = knob_find(name);
  if (!k) return FOD_ERR_ARG;
  const Knobs t = fod_knobs();
  char text[32];
  int n;
  if (k->d) n = snprintf(text, sizeof(text), "%.17g", t.*k->d);
  else if (t.*k->i == Knobs::AUTO) n = snprintf(text, sizeof(text), "auto");
  else n = snprintf(text, sizeof(text), "%d", t.*k->i);
  if (out && (size_t)n < out_bytes) memcpy(out, text, (size_t)n + 1);
  else {
    fod_set_error("knob: %zu bytes do not hold the value of %s", out_bytes, name);
    return FOD_ERR_ARG;
  }
  return FOD_OK;
}
