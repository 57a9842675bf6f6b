// C-ABI plumbing shared by every entry point: version, thread-local error text.
#include <stdarg.h>

#include "sga_common.h"

static thread_local char g_err[512] = "";

void sga_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* sga_last_error(void) { return g_err; }
extern "C" int sga_version(void) { return 105; }  // 0.1.5: + the sparse GCN route (sga_gcn_sp_dinv, sga_gcn_sp_aggregate)
extern "C" int sga_device_cus(void) { return sga_num_cus(); }
