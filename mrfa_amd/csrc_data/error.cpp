// thread-local error string + version of libmrfa_data_hip.so (include/mrfa_data_hip.h)
#include <stdarg.h>
#include <stdio.h>
#include "mrfa_data_hip.h"

static thread_local char g_data_err[512] = "";

void mrfa_data_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_data_err, sizeof(g_data_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* mrfa_data_last_error(void) { return g_data_err; }
extern "C" int mrfa_data_version(void) { return MRFA_DATA_ABI_VERSION; }
