// The packed-segment contract of the batched geometry ops (visibility.hip, scenegraph.hip, nnsearch.hip, ransac.hip, featnn.hip, fpfh.hip):
// segments packed back to back, an [n + 1] int32 prefix array on the device, and a host copy of it that is checked before any launch: prefix
// check, pointer alignment and the grid limit, all on the host (the zero-fill they share, sga_zero, is sga_common.h's).  pair_jobs.h adds the searches' job list and the device lookup.
#pragma once
#include "sga_common.h"

constexpr long long SGA_ANY = -1;                            // sga_check_prefix: do not check this bound

// How the messages speak of one prefix array: "<name> <verb> at <unit> 3", "<name> must run from 0 to <total_name>",
// "<unit> 3 has more <items> than <max_name> 7".  total_name / items / max_name may be null where that bound is never checked.
struct SgaPrefix { const char *name, *verb, *unit, *total_name, *items, *max_name; };

// The three checks of a host copy `off` of n segments, apart: an entry point that validates two arrays side by side keeps its own order.
static inline int sga_prefix_ends(const char* who, const SgaPrefix& d, const int32_t* off, int n, long long total) {
    if (total == SGA_ANY)
        SGA_CHECK_ARG(off[0] == 0, "%s: %s must start at 0", who, d.name);
    else
        SGA_CHECK_ARG(off[0] == 0 && off[n] == total, "%s: %s must run from 0 to %s", who, d.name, d.total_name);
    return SGA_OK;
}
static inline int sga_prefix_step(const char* who, const SgaPrefix& d, const int32_t* off, int i) {
    SGA_CHECK_ARG(off[i + 1] >= off[i], "%s: %s %s at %s%s%d", who, d.name, d.verb, d.unit, *d.unit ? " " : "", i);
    return SGA_OK;
}
// All of them for one array: starts at 0, ends at `total`, and segment by segment never decreases and is no longer than max_len.
// A null `off` was not provided by the caller: skipped.
static inline int sga_check_prefix(const char* who, const SgaPrefix& d, const int32_t* off, int n, long long total, long long max_len) {
    if (!off) return SGA_OK;
    if (int rc = sga_prefix_ends(who, d, off, n, total)) return rc;
    for (int i = 0; i < n; ++i) {
        if (int rc = sga_prefix_step(who, d, off, i)) return rc;
        SGA_CHECK_ARG(max_len == SGA_ANY || off[i + 1] - off[i] <= max_len, "%s: %s %d has more %s than %s %lld", who, d.unit, i, d.items, d.max_name,
                      max_len);
    }
    return SGA_OK;
}

// Every pointer of the list sits on a multiple of `bytes` (a null pointer does).
template <typename... P>
static inline bool sga_aligned(size_t bytes, const P*... p) { return ((((uintptr_t)p % bytes) == 0) && ...); }

// A one-dimensional grid of tiles x chunks x n workgroups (chunks = 1 where nothing is split) holds fewer than 2^31 of them; `advice`
// says what the caller can do about a larger one.
static inline int sga_check_grid(const char* who, long tiles, long chunks, long n, const char* advice) {
    SGA_CHECK_ARG(tiles * chunks * n < (1L << 31), "%s: %ld x %ld x %ld workgroups exceed the grid limit; %s", who, tiles, chunks, n, advice);
    return SGA_OK;
}
