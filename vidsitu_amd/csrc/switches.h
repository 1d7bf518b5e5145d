// Every VS_* environment variable the library reads: one line per switch -- name without the VS_ prefix, C type,
// default.  (The package's own switches are the table in vidsitu_amd/switches.py; INTEGRATION.md lists both, and
// tests/test_switch_list.py holds the three to each other.)
//
// vs_sw::env_NAME() is the value of VS_NAME: read once per process, at the first call, shared by every translation
// unit of the library; atoi / atoll / atof of the variable, the default when it is unset.  Clamps and roundings stay
// with the code that asks.  vs_switch_value() (txenc_ops.hip) answers from the same accessors.
//
// The table's names are used only through # and ##, never as tokens of their own: VS_CONV_SPLITK_IL is a flag macro of
// vidsitu_hip.h and WGG_JOBS a constant of conv_wgrad.hip.  Standard library only -- no HIP in this header.
#pragma once
#include <stdlib.h>

#define VS_SWITCHES(X)                  \
  X(BC32_TPW, int, 4)                   \
  X(BN_FIN2, int, 1)                    \
  X(BN_NBMAX, int, 0)                   \
  X(BN_TARGET, int, 0)                  \
  X(CONV_DEEP, int, 1)                  \
  X(CONV_HALO, int, 1)                  \
  X(CONV_KORDER_MIN, int, 2)            \
  X(CONV_PW, int, 1)                    \
  X(CONV_SPLITK_IL, int, 0)             \
  X(CONV_SPLITK_IL_NK, int, 32)         \
  X(CONV_SPLITK_IL_TILES, int, 224)     \
  X(DIRECT_BNB, int, 0)                 \
  X(DIRECT_TB, int, 0)                  \
  X(DIRECT_TPW_BLOCKS, long long, 0)    \
  X(HALO_CONFLICT_WEIGHT, double, 0.85) \
  X(LN_BWD_FUSED, int, 1)               \
  X(PW_BN, int, 0)                      \
  X(PW_DBG, int, 0)                     \
  X(PW_EDBG, int, 0)                    \
  X(PW_NSLOT, int, 0)                   \
  X(PW_OCC, int, 0)                     \
  X(STEM_PAIR, int, 1)                  \
  X(WGG_JOBS, int, 0)                   \
  X(WGG_SLOTS, int, 256)                \
  X(WGRAD_DBG, int, 0)                  \
  X(WGRAD_DEEP, int, 1)                 \
  X(WGRAD_DEEP_MINP, long long, 3000)   \
  X(WGRAD_DEEP_STAG, int, 1)            \
  X(WGRAD_S1_TILES, long long, 128)     \
  X(WGRAD_SLOTS, long long, 384)        \
  X(WGRAD_SLOTS_SMALL, long long, 512)  \
  X(WGRAD_XCD, int, 1)                  \
  X(WHATIF_LINEAR_DW, int, 0)           \
  X(WHATIF_OK, int, 0)

namespace vs_sw {
inline int parse(const char* e, int) { return atoi(e); }
inline long long parse(const char* e, long long) { return atoll(e); }
inline double parse(const char* e, double) { return atof(e); }
template <class T>
inline T read(const char* name, T dflt) {
  const char* e = getenv(name);
  return e ? parse(e, dflt) : dflt;
}
#define VS_SWITCH_ACCESSOR(name, type, dflt)                  \
  inline type env_##name() {                                  \
    static const type v = read<type>("VS_" #name, (type)dflt); \
    return v;                                                 \
  }
VS_SWITCHES(VS_SWITCH_ACCESSOR)
#undef VS_SWITCH_ACCESSOR
}  // namespace vs_sw
