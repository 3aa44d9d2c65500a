// simulator translation unit of csrc/preproc_nv12.hip (the NV12 letterbox kernels and the NV12 -> RGB8 conversion), built into a library of its own by
// tests/test_nv12.py: its extern "C" entry points (ymi_letterbox_nv12, ymi_nv12_to_rgb) are exported as they are and take HOST pointers.
#include <cstdarg>

#include "hipsim.h"
#include "hipsim.cpp"   // the scheduler lives in the library of this unit (it is built alone)

#include "../../yolort_amd/csrc/common.hpp"

namespace ymi {
static char g_err[1024];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
alignas(16) unsigned char nv12_sm[64 * 1024];
}

#include "../../yolort_amd/csrc/preproc_nv12.hip"

extern "C" const char* sim_last_error(void) { return ymi::g_err; }
