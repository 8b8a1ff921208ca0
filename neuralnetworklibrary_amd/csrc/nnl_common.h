// Shared helpers for the nnl HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/nnl.h"

#define NNL_WAVE 64

// thread-local last-error text, returned by nnl_last_error()
char* nnl_err_buf();
int nnl_set_error(int code, const char* fmt, ...);

#define NNL_CHECK_ARG(cond, ...)                                           \
  do {                                                                     \
    if (!(cond)) return nnl_set_error(NNL_ERR_INVALID_ARG, __VA_ARGS__);   \
  } while (0)

#define NNL_CHECK_HIP(expr)                                                         \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return nnl_set_error(NNL_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

#define NNL_CHECK_LAUNCH()                                                          \
  do {                                                                              \
    hipError_t _e = hipGetLastError();                                              \
    if (_e != hipSuccess)                                                           \
      return nnl_set_error(NNL_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(_e)); \
  } while (0)

static inline int64_t nnl_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Algorithm switches (NNL_* environment variables): read ONCE per site, not per launch (a getenv per call sits on
// the host's launch path).  nnl_reload_env() — exported for tests and the A/B tools — makes every site read its variable again.
int nnl_env_cached(const char* name, int dflt, int* value, int* generation);
int nnl_env_generation();          // bumped by nnl_reload_env(): caches of env-dependent plans key on it
#define NNL_ENV_INT(name, dflt) ([]() -> int { static int v_ = 0, g_ = -1; return nnl_env_cached(name, dflt, &v_, &g_); }())

// optional per-launch profiling with HIP events on the launch stream (bench.py roofline leg)
void nnl_prof_begin(int kind, hipStream_t s);
void nnl_prof_end(int kind, hipStream_t s, double work);
void nnl_prof_exec_frac(double f);   // the launch in flight executes f x its algorithmic multiplies (Winograd kernels: 1 / 1.5, 1 / 2.25)

// Route notes (debug): while nnl_debug_route_record(1) is in force on the calling thread, every launch site appends the name of what it
// launches (and the plan it picked) to a bounded thread-local buffer that nnl_debug_route_collect() hands out; off (the default) a note is
// one predictable branch.  Host code only: nothing is read from the environment, nothing allocated, no launch depends on it.
// A name is `kernel<template arguments>:plan flags`; whatever follows an `@` is a numeric detail (slice counts) that varies with the shape.
bool nnl_route_on();
void nnl_route_note(const char* name);
#define NNL_ROUTE(...)                                \
  do {                                                \
    if (nnl_route_on()) {                             \
      char route_[160];                               \
      snprintf(route_, sizeof(route_), __VA_ARGS__);  \
      nnl_route_note(route_);                         \
    }                                                 \
  } while (0)

struct NnlProfScope {
  int kind; hipStream_t s; double work;
  NnlProfScope(int k, hipStream_t st, double w) : kind(k), s(st), work(w) { nnl_prof_begin(kind, s); }
  ~NnlProfScope() { nnl_prof_end(kind, s, work); }
};

#include "block_ops.h"   // nnl_wave_sum / nnl_wave_max, the workgroup reductions and scans, nnl_sigmoid
