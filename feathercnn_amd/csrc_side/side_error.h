// side_error.h -- the error state of a side library (libfeather_<x>.so): the thread's last error, the two helpers ../csrc/common.h declares
// (fail, fail_hip: FHIP_CHECK_HIP and gemm_core.h's includers need them defined) and the accessor fhip_<x>_last_error returns.
// A side library is ONE translation unit, so the definitions below are not inline; hidden visibility keeps them private to the library,
// and each library has its own thread-local string.
#pragma once

#include <stdint.h>

#include <string>

#include "common.h"

namespace fhip
{

static thread_local std::string g_error;

int fail(int code, const char* msg)
{
    g_error = msg;
    return code;
}

int fail_hip(hipError_t e, const char* what)
{
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return FHIP_E_HIP;
}

static const char* last_error() { return g_error.c_str(); }

static bool aligned(const void* q, uintptr_t to) { return ((uintptr_t)q & (to - 1)) == 0; }

} // namespace fhip
