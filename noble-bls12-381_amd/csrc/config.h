// config.h -- the ONE place where the library reads its environment switches (round 4; 30 getenv sites before).  Every switch is read once per process, on first
// use, through env_long / env_set; the value then in force is remembered, and env_describe() (C ABI: nbls_config_describe) lists every switch asked for so far
// with its value and where it came from -- so that an A/B script can print what each side actually ran with, and a switch set after its first use (which has no
// effect) shows up as such.  Tuning values that may change at run time go through nbls_set_tuning (include/nbls.h), not through the environment.
#pragma once
#include <string>
namespace nbls {
long env_long(const char* name, long dflt);   // integer value of the variable, or dflt when it is unset or empty
bool env_set(const char* name);               // the variable is defined (whatever its value)
std::string env_describe();                   // "NAME=value (env|default) ..." of every switch read so far, in order of first use
// NBLS_FE_TAIL_CHAIN (include/nbls.h NBLS_TUNE_FE_TAIL_CHAIN) when the environment has it, else what the caller gives for its kind of context.  A switch keeps the default of
// its first reader, so the single context's 0 (nbls_internal.h) and the pool's value (nbls_multi.cpp) go through this one reader
inline unsigned fe_tail_chain_default(unsigned unset) { const long v = env_long("NBLS_FE_TAIL_CHAIN", -1); return v < 0 ? unset : (unsigned)v & 3u; }
// NBLS_FE_HEAD_CHAIN (NBLS_TUNE_FE_HEAD_CHAIN) and NBLS_INV_PRIO (NBLS_TUNE_INV_PRIO) likewise: the single context's 0 and the pool's values through one reader each
inline unsigned fe_head_chain_default(unsigned unset) { const long v = env_long("NBLS_FE_HEAD_CHAIN", -1); return v < 0 ? unset : (unsigned)v & 1u; }
inline unsigned inv_prio_default(unsigned unset) { const long v = env_long("NBLS_INV_PRIO", -1); return v < 0 ? unset : (unsigned)v & 3u; }
}  // namespace nbls
