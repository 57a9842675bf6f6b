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
extern "C" int sga_version(void) { return 103; }  // 0.1.3: + FPFH descriptors (sga_knn_lists, sga_normals, sga_spfh_counts, sga_fpfh)
extern "C" int sga_device_cus(void) { return sga_num_cus(); }
