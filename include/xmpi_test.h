/*
 * xmpi_test.h -- entry points of libxmpi.so that exist for the test suites, the verification programs under examples/ and
 * bench.py's parity leg: deterministic inputs shared with the CPU oracle, host-only self-tests and introspection of the
 * library's host logic (step tables, step programs, chunk cuts, the tuner's decision rule).  They are NOT part of the drop-in
 * boundary: the cgo shim (go/xgmi) binds include/xmpi.h only, and nothing here replaces a reference interface.
 */
#ifndef XMPI_TEST_H
#define XMPI_TEST_H

#include "xmpi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fill with the deterministic test pattern shared with the CPU oracle (oracle/xmpi_oracle.c
 * `oracle_fill`): see DESIGN.md "synthetic inputs". */
int xmpi_fill_pattern(xmpi_comm* comm, void* buf, size_t count, xmpi_dtype dtype, int pattern,
                      uint64_t seed);

/* The decision xmpi_tune applies to one row of (max-over-ranks) mean times in microseconds, <= 0 = not run: the fastest,
 * except that candidate 0 (the default) stays unless beaten by more than `margin` (host logic only). */
int xmpi_tune_decide(const double* mean_us, int n, double margin);

/* Host-only self-test of the control plane shared by the ranks of a job (no GPU call): every rank
 * of `size` calls it with the same key; exercises join, barriers, pipe counters, the mail-entry
 * states (with the direct-pull offer), the zero-copy buffer descriptors and the retire logs for
 * `rounds` rounds.  Used by the CPU test-suite with plain OS processes. */
int xmpi_ctl_selftest(const char* job_key, int rank, int size, int rounds);

/* Schedule introspection (host logic only, no GPU needed): writes the step table the executor
 * would run for (coll, algo, size, rank, count) as text into out; returns needed length.  fifo_depth 0 / oneshot_bytes
 * (size_t)-1: the library's defaults (8 slots per pipe; one-shot schedules up to 1 MiB). */
int xmpi_plan_dump(int coll, int algo, int size, int rank, int root, size_t count,
                   size_t elem_size, int channels, size_t piece_elems, int fifo_depth, size_t oneshot_bytes, char* out, size_t cap);

/* The step program of a stepped kernel (ring allreduce = 1, recursive halving + doubling = 2, ring allgather = 3,
 * binary-tree bcast = 4, binary-tree reduce = 5; form 0 = pull, 1 = push; in_place: the ranks' send buffers are their receive
 * buffers) for one rank and ring channel, as text, from the very function the kernel runs (mpi_amd/csrc/sched_steps.h; host
 * logic only, no GPU needed: the CPU test-suite executes all ranks' programs under random interleavings).  Returns the needed
 * length. */
int xmpi_sched_dump(int sched, int form, int in_place, int size, int rank, int root, int pieces, size_t count, size_t elem_size,
                    int nchan, int channel, char* out, size_t cap);
/* Bytes of the landing block `rank` lends to the push form of that schedule (0: none). */
size_t xmpi_sched_land_bytes(int sched, int in_place, int size, int rank, int root, size_t count, size_t elem_size);

/* xmpi_alltoallv with ranks that meet on the host moves its blocks in `size` rounds of disjoint pairs: the partner of `rank` in
 * round `round` (a rank may be its own).  Host logic only; -1 for arguments out of range. */
int xmpi_alltoallv_partner(int round, int rank, int size);

/* Chunk j of a count-element buffer cut for `size` ranks the way the zero-copy collectives cut it
 * (16-byte aligned boundaries): element offset and length.  Host logic only. */
int xmpi_zc_chunk(size_t count, size_t elem_size, int size, int j, size_t* elem_off, size_t* elem_cnt);

/* The batch launchers of the staged step tables (mpi_amd/csrc/kernels.h launch_reduce2_batch / launch_copy_batch) on local
 * buffers, n <= 16 segments in one call: dst[i] = a[i] op b[i] over counts[i] elements, resp. dst[i] = src[i] over bytes[i] bytes,
 * and the same once more into dst2[i].  dst2 may be NULL or hold NULL entries; for the reduction dst[i] may be NULL as well (the
 * result is only forwarded), and dst[i] may be a[i] or b[i] (dst2[i] then still holds the fold of the untouched operands). */
int xmpi_reduce_local_batch(xmpi_comm* comm, void* const* dst, void* const* dst2, const void* const* a, const void* const* b,
                            const size_t* counts, int n, xmpi_dtype dtype, xmpi_op op);
int xmpi_copy_local_batch(xmpi_comm* comm, void* const* dst, void* const* dst2, const void* const* src, const size_t* bytes, int n);

/* Host-only self-test of xmpi_malloc's block bookkeeping (no GPU call): `rounds` random allocate /
 * free operations on a synthetic arena; 0 = blocks never overlapped, stayed aligned and coalesced
 * back into one free block, otherwise the number of the failed check. */
int xmpi_heap_selftest(uint64_t seed, int rounds);

/* Row `index` of the library's one table of knobs and diagnostics (mpi_amd/csrc/params.cpp): what xmpi_set_param / xmpi_get_param
 * call it (NULL: none; with XMPI_PARAM_PATTERN: a prefix), the environment variable xmpi_init reads it from (NULL: none), its fixed
 * default and its range [lo, hi].  XMPI_ERR_ARG past the last row.  Needs no communicator: what
 * INTEGRATION.md section 5 says is held to this by the CPU suite. */
#define XMPI_PARAM_WRITABLE 1        /* xmpi_set_param accepts it */
#define XMPI_PARAM_BOOLEAN 2         /* any value but 0 is 1 */
#define XMPI_PARAM_LAYOUT_DEFAULT 4  /* no fixed default: decided where the job's layout is known (*dflt means nothing) */
#define XMPI_PARAM_READ_ONLY 8       /* xmpi_set_param refuses it */
#define XMPI_PARAM_PATTERN 16        /* a family of names that begin with *name */
#define XMPI_PARAM_ENV_AUTO 32       /* the environment (only) may say -1 = decide later; below lo means the same */
int xmpi_param_info(int index, const char** name, const char** env, long* dflt, long* lo, long* hi, int* flags);

#ifdef __cplusplus
}
#endif
#endif /* XMPI_TEST_H */
