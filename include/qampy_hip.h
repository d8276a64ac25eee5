/*
 * qampy_hip.h - C ABI of libqampy_hip.so: hand-written HIP (gfx950 / MI355X) kernels behind QAMpy's compiled hot path.
 *
 * What this replaces.  QAMpy's only native code are two pythran-compiled modules; their `#pythran export` lines are the
 * de-facto FFI contract of the hot path (paths relative to the QAMpy tree):
 *   qampy/core/equalisation/pythran_equalisation.py:33-36    apply_filter_to_signal  {f32,f64,c64,c128}
 *   qampy/core/equalisation/pythran_equalisation.py:78-79    train_equaliser_realvalued {f32,f64}
 *   qampy/core/equalisation/pythran_equalisation.py:128-129  train_equaliser {c64,c128}
 *   qampy/core/equalisation/pythran_equalisation.py:304-305  make_decision {c64,c128}
 *   qampy/core/pythran_dsp.py:45-46                          bps {c64,c128}
 *   qampy/core/pythran_dsp.py:133-136                        select_angles {f32,f64}
 * Call sites that bind to them: qampy/core/equalisation/equalisation.py:177,180,555,557;
 * qampy/core/phaserecovery.py:28-29,149-150; qampy/core/signal_quality.py:26.
 *
 * Conventions
 *   - plain pointers and sizes only; complex data is interleaved (re, im) exactly like numpy complex64/complex128;
 *   - all arrays C-contiguous, row-major, shapes given in the comments;
 *   - every function returns a status code (QH_OK == 0); the library never frees or keeps caller memory;
 *   - `qh_*`      : pointers are HOST memory (numpy arrays); the call stages through HBM and is synchronous;
 *   - `qh_*_dev`  : array pointers are DEVICE memory obtained from qh_malloc; the call only enqueues work on the
 *                   library's stream (use qh_sync / events).  Small control arrays (`modes`) stay host pointers.
 *   - method ids are the QH_M_* / QH_RM_* enums below (the reference matches strings, pythran_equalisation.py:131-152).
 *
 * Semantics are those of the reference run sequentially (OMP_NUM_THREADS=1): modes are processed in the order given
 * and, with adaptive != 0, the adapted step size is carried from one mode into the next.
 */
#ifndef QAMPY_HIP_H
#define QAMPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ABI version: bumped whenever an entry point changes its argument list or a public struct its layout, so that a caller
 * built against another header fails loudly (compare with qh_abi_version() at load time) instead of passing shifted
 * arguments.  History: 1 = round 1; 2 = round 2 (qh_bps_recover_*_dev gained `angles`, qh_train_equaliser_*_pit_dev takes
 * (gram, opts, report), the *_seg_dev entry points were removed - unversioned at the time); 3 = round 3 (qh_pit_opts:
 * start, dev_safety; qh_pit_report: deviation[]); 4 = qh_pit_opts: adaptive; 11 = signal-quality metrics (qh_metrics_*,
 * qh_soft_l_value_demapper_*, qh_estimate_snr_*, qh_cal_mi_mc_*). */
#define QH_ABI_VERSION 11
int qh_abi_version(void);

/* ---- status codes (python shim: 1,2 -> ValueError, 3,4 -> RuntimeError) */
#define QH_OK 0
#define QH_ERR_METHOD 1   /* unknown method id   (reference: ValueError, pythran_equalisation.py:151-152) */
#define QH_ERR_ARG 2      /* inconsistent sizes  (reference: asserts that the compiled build drops)          */
#define QH_ERR_HIP 3      /* HIP runtime failure, text in qh_last_error()                                      */
#define QH_ERR_NODEVICE 4 /* no usable gfx950 device                                                           */

/* ---- complex trainer methods, pythran_equalisation.py:131-150 */
enum { QH_M_CMA = 0, QH_M_CMA2, QH_M_SGNCMA, QH_M_MCMA, QH_M_RDE, QH_M_MRDE, QH_M_SBD, QH_M_MDDMA, QH_M_DD, QH_M_SBD_DATA };
/* ---- real-valued trainer methods, pythran_equalisation.py:81-88 */
enum { QH_RM_CMA = 0, QH_RM_SGNCMA, QH_RM_DD, QH_RM_DD_DATA };

/* ---- device / runtime --------------------------------------------------------------------------------------- */
int qh_device_count(int *count);
int qh_init(int device);                       /* select the device and create the library streams; idempotent for the same device; ONE device
                                                * per process: a second call with another index fails with QH_ERR_ARG (run one process per GPU) */
int qh_device_name(char *buf, size_t n);
const char *qh_last_error(void);
int qh_sync(void);                             /* wait for the library stream */
int qh_malloc(void **dptr, size_t bytes);
int qh_free(void *dptr);
int qh_memset(void *dptr, int value, size_t bytes);
int qh_memcpy_h2d(void *dptr, const void *hptr, size_t bytes);
int qh_memcpy_d2h(void *hptr, const void *dptr, size_t bytes);
int qh_memcpy_d2d(void *dst, const void *src, size_t bytes);
/* Pinned host memory from a library pool + asynchronous copies on the current library stream (ABI 8): the mirrored host layers return
 * ndarrays that view pooled pinned buffers (one DMA at the PCIe rate, no bounce copy, no first-touch page faults), and copy a stage's
 * error trace back while the next stage trains.  qh_stream_sync waits for the current stream only. */
int qh_pinned_alloc(void **hptr, size_t bytes);
int qh_pinned_free(void *hptr);
int qh_memcpy_h2d_async(void *dptr, const void *hptr, size_t bytes);
int qh_memcpy_d2h_async(void *hptr, const void *dptr, size_t bytes);
int qh_stream_sync(void);
/* Threading: the library keeps per-process state (current device and stream, grow-only scratch buffers, trainer selection) and
 * is meant to be driven by ONE host thread, like the reference's extension modules under the GIL; error text is per thread.
 * qh_release_scratch frees the grow-only scratch buffers (Gram tables above all - up to qh_set_gram_budget_gb) after
 * draining both streams; they are re-allocated on demand. */
int qh_release_scratch(void);
int qh_thread_release(void);                   /* destroy the calling thread's streams and scratch buffers (they come back on the next call): a worker
                                                  thread before it ends, the main thread at exit (qampy_amd._lib registers it with atexit) */
/* Three library streams.  Every entry point enqueues on the CURRENT one (0 after qh_init); qh_use_stream(0..2) switches it,
 * qh_stream_wait_event makes the current stream wait for an event recorded on another one, qh_sync drains all of them.
 * Streams 0 and 1 are equals (a tier-b trainer puts its eigen-solver on whichever of the two is not current); stream 2 has the
 * lowest queue priority and is meant for chip-wide streaming work (phase search of capture k) overlapped with the latency-bound
 * trainers of capture k+1 on stream 0 (ResidentReceiver.run(overlap=True)).
 * Streams, scratch buffers and the events of the tier-b solver are PER HOST THREAD: a thread that calls into the library gets its own
 * set on first use (same device), so several captures can be in flight on one GPU, one driving thread each (pipeline.py ReceiverGroup);
 * qh_sync / qh_release_scratch act on the calling thread's set.  Device memory and the staging pool are per process.
 * Within a thread scratch buffers are per library, not per stream: overlap only stages that use different ones (trainers + Gram tables on
 * one stream; filter, phase search and SER harness on the other - what ChannelBank.run_pipelined does). */
int qh_use_stream(int idx);
int qh_stream_wait_event(void *ev);
int qh_stream_handle(void **stream);           /* the current library stream as a hipStream_t, for collectives enqueued next to the kernels (RCCL: qampy_amd/comm.py) */
/* HIP events recorded on the current library stream (bench.py measures kernel time with these) */
int qh_event_create(void **ev);
int qh_event_destroy(void *ev);
int qh_event_record(void *ev);
int qh_event_elapsed_ms(void *start, void *stop, float *ms);   /* synchronises on `stop` */

/* ---- train_equaliser (complex) ----------------------------------------------------------------------------------
 *   E        (nmodes, L)                 input field
 *   mu       in/out step size (the adapted value is returned when adaptive != 0)
 *   adaptive 0 fixed step; 1 adapt_step with the reference's sequential semantics (mu carried from sweep to sweep and
 *            from mode to mode, pythran_equalisation.py:162-172 with one thread); 2 (extension) one step size per mode:
 *            exactly the result of one call per selected mode from the initial mu, modes trained concurrently, mu out =
 *            the last mode's (the compiled reference's OpenMP threads share and race on mu; 2 is its deterministic stand-in)
 *   wx       (nmodes, nmodes, ntaps)     taps, updated in place
 *   modes    (nsel,) int64               output modes to train, processed in this order
 *   symbols  (nmodes, nsy)               per-method constants / alphabet / training symbols
 *   err      (nmodes, TrSyms*Niter)      out; rows of unselected modes are zeroed
 * Requires (TrSyms-1)*os + ntaps <= L, nsel >= 1, modes[i] < nmodes, and nsy >= TrSyms for QH_M_SBD_DATA.
 */
int qh_train_equaliser_c64(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, float *mu, void *wx,
                           int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols, int64_t nsy,
                           int method, void *err);
int qh_train_equaliser_c128(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, double *mu, void *wx,
                            int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols, int64_t nsy,
                            int method, void *err);
/* device-resident: E, wx, symbols, err, mu are device pointers; err is NOT zeroed for unselected modes unless zero_err */
int qh_train_equaliser_c64_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, float *mu_dev,
                               void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols,
                               int64_t nsy, int method, void *err, int zero_err);
int qh_train_equaliser_c128_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, double *mu_dev,
                                void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols,
                                int64_t nsy, int method, void *err, int zero_err);

/* Gram terms of the look-ahead trainer: G(l, i) = sum_f conj(x_l[f]) x_i[f] for the 127 steps after l, laid out for the
 * kernel.  They depend on the capture only, so one build serves every mode, stage and sweep over the same
 * (E, os, ntaps, TrSyms).  The buffer is library-owned scratch: valid until the next qh_gram_build_* call; pass it to
 * qh_train_equaliser_*_gram_dev, or pass NULL there (and to the plain _dev / host entry points) to build it internally. */
int qh_gram_build_c64_dev(const void *E, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void **gram);
int qh_gram_build_c128_dev(const void *E, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void **gram);
int qh_train_equaliser_c64_gram_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, float *mu_dev,
                                    void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols,
                                    int64_t nsy, int method, void *err, int zero_err, const void *gram);
int qh_train_equaliser_c128_gram_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, double *mu_dev,
                                     void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols,
                                     int64_t nsy, int method, void *err, int zero_err, const void *gram);

/* Batch of independent equaliser runs on `nwin` windows E[:, win_start[v] : win_start[v] + win_len] of one capture, all from
 * the same initial taps wx0 and step size mu - what the frame synchronisation of the pilot receiver does in a Python loop
 * (qampy/core/pilotbased_receiver.py:395-400).  Results are those of nwin separate qh_train_equaliser_* calls; the windows
 * run concurrently (one wavefront each).  wx_out (nwin, nmodes, nmodes, ntaps), err (nwin, nmodes, TrSyms*Niter), mu_out (nwin). */
int qh_train_equaliser_windows_c64(const void *E, int nmodes, int64_t L, const int64_t *win_start, int nwin, int64_t win_len,
                                   int64_t TrSyms, int Niter, int os, float mu, const void *wx0, int ntaps, const int64_t *modes, int nsel,
                                   int adaptive, const void *symbols, int64_t nsy, int method, void *wx_out, void *err, float *mu_out);
int qh_train_equaliser_windows_c128(const void *E, int nmodes, int64_t L, const int64_t *win_start, int nwin, int64_t win_len,
                                    int64_t TrSyms, int Niter, int os, double mu, const void *wx0, int ntaps, const int64_t *modes, int nsel,
                                    int adaptive, const void *symbols, int64_t nsy, int method, void *wx_out, void *err, double *mu_out);

/* Search form of the window batch: the error traces stay in HBM; out come var (nmodes, nwin) = variance of every window's
 * error trace per mode (np.var of the complex row), best (nmodes) = window with the smallest variance per mode (first
 * minimum) and wx_best (nmodes, nmodes, nmodes, ntaps) = the tap sets of those windows. */
int qh_train_equaliser_windows_search_c64(const void *E, int nmodes, int64_t L, const int64_t *win_start, int nwin, int64_t win_len,
                                          int64_t TrSyms, int Niter, int os, float mu, const void *wx0, int ntaps, const int64_t *modes, int nsel,
                                          int adaptive, const void *symbols, int64_t nsy, int method, double *var, int32_t *best, void *wx_best);
int qh_train_equaliser_windows_search_c128(const void *E, int nmodes, int64_t L, const int64_t *win_start, int nwin, int64_t win_len,
                                           int64_t TrSyms, int Niter, int os, double mu, const void *wx0, int ntaps, const int64_t *modes, int nsel,
                                           int adaptive, const void *symbols, int64_t nsy, int method, double *var, int32_t *best, void *wx_best);

/* ---- train_equaliser_realvalued: same layout with real arrays, update without conjugate ---------------------- */
int qh_train_equaliser_real_f32(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, float *mu, void *wx,
                                int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols, int64_t nsy,
                                int method, void *err);
int qh_train_equaliser_real_f64(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, double *mu, void *wx,
                                int ntaps, const int64_t *modes, int nsel, int adaptive, const void *symbols, int64_t nsy,
                                int method, void *err);

/* ---- apply_filter_to_signal -------------------------------------------------------------------------------------
 *   out (nsel, N), N = (L - ntaps + 1) / os ;  out[j, i] = sum_k sum_t E[k, i*os + t] * wx[modes[j], k, t]
 */
int qh_apply_filter_c64(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                        int nsel, void *out);
int qh_apply_filter_c128(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                         int nsel, void *out);
int qh_apply_filter_f32(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                        int nsel, void *out);
int qh_apply_filter_f64(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                        int nsel, void *out);
int qh_apply_filter_c64_dev(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                            int nsel, void *out);
int qh_apply_filter_c128_dev(const void *E, int nmodes, int64_t L, int os, const void *wx, int ntaps, const int64_t *modes,
                             int nsel, void *out);
/* The launch form a call of these sizes takes (is_complex != 0: the complex kernel; elem_real_bytes 4 or 8): output symbols per thread
 * (*per_thread: 4, or 1 when four rows per thread do not fit the LDS) and per workgroup (*tile), the dynamic LDS of a workgroup (*lds_bytes)
 * and the workgroups along the selected modes (*grid_y: pairs of modes for the complex kernel, one row each for the real one).  QH_ERR_ARG
 * exactly when the entry points above refuse the same sizes.  Any pointer may be NULL.  No device needed. */
int qh_apply_plan(int is_complex, int elem_real_bytes, int nmodes, int os, int ntaps, int nsel, int *per_thread, int *tile, int64_t *lds_bytes,
                  int *grid_y);

/* ---- bps: blind phase search index ---------------------------------------------------------------------------
 *   E (L,) one mode; testangles (p, A) real with p == 1 (one grid) or p == L (per-symbol grid); symbols (M,)
 *   idx (L,) int32 out: first arg-min over the A angles of the 2N-symbol windowed min-distance sum; 0 in [0,N) and [L-N,L)
 */
int qh_bps_c64(const void *E, int64_t L, const void *testangles, int64_t p, int A, const void *symbols, int M, int N,
               int32_t *idx);
int qh_bps_c128(const void *E, int64_t L, const void *testangles, int64_t p, int A, const void *symbols, int M, int N,
                int32_t *idx);
int qh_bps_c64_dev(const void *E, int64_t L, const void *testangles, int64_t p, int A, const void *symbols, int M, int N,
                   int32_t *idx);
int qh_bps_c128_dev(const void *E, int64_t L, const void *testangles, int64_t p, int A, const void *symbols, int M, int N,
                    int32_t *idx);

/* device-resident carrier recovery of the host layer qampy/core/phaserecovery.py:145-159 for `nm` modes at once:
 *   idx = bps(E[m], grid); ph = grid[idx]; ph[N:-N] = unwrap(4 ph)/4; Eout = E * exp(1j ph).
 * angles: the grid (A,) real in HBM, as the host builds it (np.linspace(-pi/4, pi/4, A, endpoint=False) in double, cast to
 * the signal's precision), or NULL for a grid formed on the device.  np.unwrap's jump decisions are evaluated with numpy's own
 * operations on the grid values (a jump of exactly half the range depends on their rounding), the running correction is an
 * exact integer prefix sum.  With the host's grid ph carries exactly the quarter turns np.unwrap gives the host layer.  A grid
 * formed on the device may differ from the host's in the last bit of an entry: a jump of exactly A/2 entries then follows
 * numpy's rule on the DEVICE's values and may be corrected where the host's is not, or the reverse - a whole quarter turn on
 * every later symbol of the row.  Pass the host's grid where that matters.
 * E, Eout (nm, L) complex; ph (nm, L) real; idx (nm, L) int32 scratch/out. */
int qh_bps_recover_c64_dev(const void *E, int nm, int64_t L, const void *angles, int A, const void *symbols, int M, int N, int32_t *idx,
                           void *ph, void *Eout);
int qh_bps_recover_c128_dev(const void *E, int nm, int64_t L, const void *angles, int A, const void *symbols, int M, int N, int32_t *idx,
                            void *ph, void *Eout);
/* the same in `nparts` calls (ABI 9): parts 0 .. nparts - 2 search a run of the signal each, part nparts - 1 searches the rest, unwraps and de-rotates.
 * A receiver that processes capture after capture enqueues one part beside each relaxation pass of the NEXT capture's training (qh_pit_opts.on_pass):
 * a part of an eighth of the search is one wave per SIMD: it starts with a pass's trainer and lives on the issue slots that pass leaves, where the whole search at once slows a pass by a third.
 * Same kernels on the same data: the results do not depend on nparts.  The parts of one search are issued by one thread, in order, on one stream,
 * with no other phase search of that thread in between. */
int qh_bps_recover_part_c64_dev(const void *E, int nm, int64_t L, const void *angles, int A, const void *symbols, int M, int N, int32_t *idx,
                                void *ph, void *Eout, int part, int nparts);
int qh_bps_recover_part_c128_dev(const void *E, int nm, int64_t L, const void *angles, int A, const void *symbols, int M, int N, int32_t *idx,
                                 void *ph, void *Eout, int part, int nparts);

/* Two-stage blind phase search (qampy/core/phaserecovery.py:222-288) of `nm` modes at once, resident in HBM: the coarse search over the
 * grid `angles` (A,) as above, then for symbol j the B angles fine[j, a] = (R)((double)angles[idx1[j]] + off[a]) with
 * off[a] = linspace(-B/2, B/2, B)[a] / (B A) * pi/2 (formed by the library in double), searched with the window and edge rule of the
 * per-symbol grid of qh_bps_*; ph = unwrap(4 fine[j, idx2[j]]) / 4 over the WHOLE row (no edge exclusion; the wrap counts are an exact
 * integer prefix sum); Eout = E * exp(1j ph).  Nothing of size L x B is formed.  E, Eout (nm, L) complex, Eout != E; ph (nm, L) real;
 * idx1, idx2 (nm, L) int32 out; angles may be NULL (grid formed on the device).  A >= 1, 1 <= B <= 64, N >= 1; a window 2N that does not
 * fit the kernel's LDS ring (2N * 256 B complex64, 2N * 512 B complex128, of 120 KiB) is QH_ERR_ARG. */
int qh_bps_twostage_recover_c64_dev(const void *E, int nm, int64_t L, const void *angles, int A, int B, const void *symbols, int M, int N,
                                    int32_t *idx1, int32_t *idx2, void *ph, void *Eout);
int qh_bps_twostage_recover_c128_dev(const void *E, int nm, int64_t L, const void *angles, int A, int B, const void *symbols, int M, int N,
                                     int32_t *idx1, int32_t *idx2, void *ph, void *Eout);

/* ---- comp_freq_offset (pilot receiver; qampy/core/phaserecovery.py:435-473): out[k, n] = E[k, n] exp(-2 pi i (n + 1) fo[k] / os),
 * fo (nmodes,) in units of the symbol rate, E / out (nmodes, L) host arrays */
int qh_comp_freq_offset_c64(const void *E, int nmodes, int64_t L, const double *fo, int os, void *out);
int qh_comp_freq_offset_c128(const void *E, int nmodes, int64_t L, const double *fo, int os, void *out);
/* The same with E, fo and out in DEVICE memory (fo: what qh_find_freq_offset_*_dev wrote); out == E is allowed.  Enqueued on the current stream. */
int qh_comp_freq_offset_c64_dev(const void *E, int nmodes, int64_t L, const double *fo, int os, void *out);
int qh_comp_freq_offset_c128_dev(const void *E, int nmodes, int64_t L, const double *fo, int os, void *out);
/* ---- find_freq_offset (qampy/core/phaserecovery.py:385-433): blind frequency-offset estimate of every row of E (nmodes, L) from the peak of
 *     P[k] = sum_b |FFT_N(E[row, b N : (b + 1) N] ** 4)[k]|^2,   b = 0 .. blocks - 1,   N = fft_size,
 * a power of two from 2^8 to 2^20 (anything else: QH_ERR_ARG).  blocks = 1 is the reference's estimator: a row shorter than N is zero-padded,
 * of a longer one the first N samples are read.  blocks > 1 (a Welch average) needs blocks * fft_size <= L.  Per row, bin = the first maximum
 * of P; fo_out[row] = fftfreq(N, 1 / os)[bin] / 4 in units of the symbol rate, and with average != 0 every row gets the mean over the rows.
 * stats_out (nmodes, 3), optional: bin, P[bin], sum_k P[k].  spectrum_out (nmodes, N), optional: P in the signal's real type, in bin order.
 * Sums are formed in a fixed order without atomics: a repeated call is bit-identical.  The _dev forms take device pointers, read nothing back
 * and are enqueued on the current stream; the others take host pointers. */
int qh_find_freq_offset_c64_dev(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                                void *spectrum_out);
int qh_find_freq_offset_c128_dev(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                                 void *spectrum_out);
int qh_find_freq_offset_c64(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                            void *spectrum_out);
int qh_find_freq_offset_c128(const void *E, int nmodes, int64_t L, int os, int fft_size, int blocks, int average, double *fo_out, double *stats_out,
                             void *spectrum_out);
/* ---- viterbiviterbi (qampy/core/phaserecovery.py:40-79): Viterbi-Viterbi carrier recovery of every row of E (nmodes, L), M-PSK, 2 <= M <= 64,
 * over windows of N samples, 1 <= N <= min(L, 1024) (anything else: QH_ERR_ARG).  z = (E / |E|)^M in the signal's precision (a zero sample
 * counts as 1), window sums in double, their angles unwrapped as numpy does; trace (nmodes, L - N + 1), in the signal's real type, is
 * (unwrapped - pi) / M formed in double, and Eout[row, o + k] = E[row, o + k] exp(-j trace[row, k]) with o = (N - 1) / 2; the other N - 1
 * samples of every row of Eout are zero.  Device pointers, nothing read back, enqueued on the current stream. */
int qh_vv_recover_c64_dev(const void *E, int nmodes, int64_t L, int N, int M, void *trace, void *Eout);
int qh_vv_recover_c128_dev(const void *E, int nmodes, int64_t L, int N, int M, void *trace, void *Eout);
/* ---- phase_partition_16qam (qampy/core/phaserecovery.py:292-382): 16-QAM carrier recovery by QPSK partitioning of every row of E (nmodes, L)
 * in blocks of Nblock samples, 1 <= Nblock <= 4096 (the last block may be short).  Ring thresholds from cal_s0(E, 1.32) of the row and the class
 * of a sample in double, fourth powers in the signal's precision, block sums in double.  trace (nmodes, L), in the signal's real type, is the
 * reference's, mode for mode: unwrap(theta) / 4 - pi / 4.  Eout = E exp(-j trace), every mode by its own trace - NOT the reference's field,
 * which rotates every mode by four times the last mode's estimate.  Device pointers, nothing read back, current stream. */
int qh_partition16_recover_c64_dev(const void *E, int nmodes, int64_t L, int Nblock, void *trace, void *Eout);
int qh_partition16_recover_c128_dev(const void *E, int nmodes, int64_t L, int Nblock, void *trace, void *Eout);
/* Tail of pilot_based_cpe_new (qampy/core/pilotbased_receiver.py:318-327): the averaged pilot phases kph (nmodes, nk) at the symbol
 * positions knots (nk, strictly increasing - the caller's duty: two equal knots divide by zero) interpolated linearly to every symbol by
 * np.interp's expression in double, slope * (i - knot) + phase with the product and the sum each rounded (numpy's result to the bit
 * where numpy's build does not fuse the two), and taken out: out = E exp(-1j trace); trace in the
 * signal's complex dtype like the reference returns it.  Host arrays. */
int qh_pilot_phase_trace_c64(const void *E, int nmodes, int64_t L, const int64_t *knots, const double *kph, int nk, void *out, void *trace);
int qh_pilot_phase_trace_c128(const void *E, int nmodes, int64_t L, const int64_t *knots, const double *kph, int nk, void *out, void *trace);

/* ---- chromatic dispersion (qampy/core/equalisation/equalisation.py:596-669 CDcomp, qampy/core/impairments.py:673-703 add_dispersion):
 * every row of E (nmodes, L) filtered by the all-pass H(w) = exp(j (c2 w^2 + c1 w + c0)), w = 2 pi k / N the digital angular frequency of
 * fftfreq bin k of a block FFT of size N (a power of two, 256 .. 8192, both precisions).  mode 0, circular: overlap-save of blocks of N / 2
 * output samples with N / 4 of halo on each side, the input taken modulo L; out (nmodes, L); N == L is one exact circular transform per row.
 * mode 1, linear: the zero-padded overlap-add of CDcomp with N > 0 (blocks of N / 2 input samples at offset N / 4 of N zeros); out
 * (nmodes, (L / (N / 2)) * (N / 2)).  out must not alias E.  Deterministic. */
int qh_cd_filter_c64(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out);
int qh_cd_filter_c128(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out);
int qh_cd_filter_c64_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out);
int qh_cd_filter_c128_dev(const void *E, int nmodes, int64_t L, int N, double c2, double c1, double c0, int mode, void *out);

/* ---- channel impairments on a resident field (qampy/core/impairments.py:29-328; csrc/impair.hip).
 * qh_impair_pointwise: out[m, n] = E[m, n] exp(j (phi[m, n] + 2 pi n freq)) + sigma w[m, n], every term optional, E / out (nmodes, L), out == E
 * allowed.  w: complex Gaussian noise of unit variance split over I and Q, Philox4x32-10 keyed by `seed` with the counter (n low, n high,
 * mode, 2) - a draw depends on (seed, mode, n) only; complex64 draws in float with the fast intrinsics, complex128 from 53-bit uniforms in
 * double.  noise_mode 0: no noise; 1: sigma = noise; 2: sigma = noise sqrt(mean |E|^2) with the mean over ALL modes, reduced on the device
 * (change_snr: noise = 10^(-snr / 20) sqrt(fs / fb)).  have_phase: phi is a Wiener process per mode, increments N(0, phase_var) from counter
 * stream 1, accumulated like np.cumsum in double; trace (nmodes, L) doubles, optional, receives phi.  have_freq: freq in turns per sample
 * (fo / fs), n freq reduced modulo one turn in double.  At most three dependent launches; no atomics, a repeated call is bit-identical.
 * The _dev forms take device pointers, read nothing back and are enqueued on the current stream; the others take host pointers. */
int qh_impair_pointwise_c64_dev(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq,
                                double freq, uint64_t seed, double *trace, void *out);
int qh_impair_pointwise_c128_dev(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq,
                                 double freq, uint64_t seed, double *trace, void *out);
int qh_impair_pointwise_c64(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                            uint64_t seed, double *trace, void *out);
int qh_impair_pointwise_c128(const void *E, int nmodes, int64_t L, int noise_mode, double noise, int have_phase, double phase_var, int have_freq, double freq,
                             uint64_t seed, double *trace, void *out);
/* The phase alone: out (nmodes, L) doubles in DEVICE memory receives the Wiener process of qh_impair_pointwise (cumulative != 0) or its raw
 * increments (cumulative == 0), drawn as the complex64 (_c64) or the complex128 (_c128) pass draws them. */
int qh_phase_noise_c64_dev(double *out, int nmodes, int64_t L, double phase_var, uint64_t seed, int cumulative);
int qh_phase_noise_c128_dev(double *out, int nmodes, int64_t L, double phase_var, uint64_t seed, int cumulative);
/* rotate_field: out = [[cos, -sin], [sin, cos]] E for the two rows of E (2, L); nmodes != 2 is QH_ERR_ARG; out == E allowed. */
int qh_rotate_field_c64_dev(const void *E, int nmodes, int64_t L, double theta, void *out);
int qh_rotate_field_c128_dev(const void *E, int nmodes, int64_t L, double theta, void *out);
/* apply_PMD_to_field: R(-theta) diag(H, conj H) R(theta) E with H = exp(-j w dgd / 2), dgd in SAMPLES (t_dgd fs), w the digital angular
 * frequency of the block's fftfreq grid.  L a power of two from 256 to 8192: one exact circular transform per row; any other L:
 * overlap-save with blocks of 8192 (4096 kept, 2048 of halo on each side, the input taken modulo L), which truncates the tail of a
 * fractional delay.  nmodes != 2 is QH_ERR_ARG; out must not alias E.  Two launches. */
int qh_apply_pmd_c64_dev(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out);
int qh_apply_pmd_c128_dev(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out);
int qh_apply_pmd_c64(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out);
int qh_apply_pmd_c128(const void *E, int nmodes, int64_t L, double theta, double dgd, void *out);
/* add_modal_delay: row m of out is row m of E rolled by delays[m] whole samples (np.roll); delays (nmodes,) in HOST memory; out must not
 * alias E.  Two copies per row on the current stream. */
int qh_modal_delay_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *delays, void *out);
int qh_modal_delay_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *delays, void *out);

/* ---- transmitter response on a resident field (qampy/core/impairments.py:370-671, qampy/core/filter.py:86-147; csrc/txresp.hip).  All
 * entry points below work on (nmodes, L) complex fields in DEVICE memory, enqueue on the calling thread's current stream, read nothing back
 * and do not synchronise; out == E is allowed everywhere.
 * qh_row_extrema: ext[2 m] = max |re|, ext[2 m + 1] = max |im| of row m, doubles in DEVICE memory; 1 to 1024 modes, L >= 1.  Two launches,
 * bit-reproducible. */
int qh_row_extrema_c64_dev(const void *E, int nmodes, int64_t L, double *ext);
int qh_row_extrema_c128_dev(const void *E, int nmodes, int64_t L, double *ext);
/* The DAC's point-wise part, stages a mask of 1 (clip), 2 (quantise), 4 (ENOB noise), applied in that order (sim_DAC_response):
 *   clip      every row scaled to +-1 / clip_rat by its own maximum max(max |re|, max |im|), re and im clamped to +-1
 *   quantise  every row scaled to +-1 by its own maximum; level index = number of thresholds -1 + k d, k = 1 .. 2^bits - 1, d = 2 / 2^bits,
 *             that are <= the value; out = (-1 + d / 2 + index d) times the maximum over ALL rows of the quantiser's input (1 to 16 bits)
 *   noise     sigma = sqrt(2 (x_max / 2^(enob - 1))^2 / 12), x_max over all rows of this stage's input, added as
 *             qh_impair_pointwise(noise_mode 1, sigma, seed) adds it
 * ext: the row extrema of E (qh_row_extrema), or NULL: formed here (two more launches).  stages = 0 copies E to out. */
int qh_dac_pointwise_c64_dev(const void *E, int nmodes, int64_t L, const double *ext, int stages, double clip_rat, int quant_bits, double enob, uint64_t seed,
                             void *out);
int qh_dac_pointwise_c128_dev(const void *E, int nmodes, int64_t L, const double *ext, int stages, double clip_rat, int quant_bits, double enob, uint64_t seed,
                              void *out);
/* scipy.signal.sosfilt(sos, E, axis=-1) with zero initial state, every row on its own, exact and parallel in time.  sos: nsec (1 to 4) rows
 * of b0 b1 b2 a0 a1 a2 with a0 = 1, doubles in HOST memory.  P: the (2 nsec) x (2 nsec) matrix, row-major doubles in HOST memory, that maps
 * the cascade's state (z0, z1 of section 0, then of section 1, ...) over *chunk zero-input samples (qh_sos_geometry).  Coefficients and state
 * are double in both precisions.  Three launches (one for L <= *tile). */
int qh_sosfilt_c64_dev(const void *E, int nmodes, int64_t L, const double *sos, int nsec, const double *P, void *out);
int qh_sosfilt_c128_dev(const void *E, int nmodes, int64_t L, const double *sos, int nsec, const double *P, void *out);
/* Samples per lane (*chunk) and per workgroup (*tile) of qh_sosfilt; either pointer may be NULL.  No device needed. */
int qh_sos_geometry(int *chunk, int *tile);
/* ideal_amplifier_response (have_amp != 0: x / max * tgt_v, the maximum over all rows from ext, or formed here when ext is NULL), then
 * modulator_response.  prm: 8 doubles in HOST memory - dcbias (I, Q), gfactr (I, Q), cfactr (I, Q), dcbias_out, gfactr_out. */
int qh_modulator_c64_dev(const void *E, int nmodes, int64_t L, const double *ext, int have_amp, double tgt_v, const double *prm, void *out);
int qh_modulator_c128_dev(const void *E, int nmodes, int64_t L, const double *ext, int have_amp, double tgt_v, const double *prm, void *out);

/* ---- polyphase resampling (qampy/core/resample.py:37-127 resample_poly / rrcos_resample, qampy/core/filter.py:177-212 rrcos_pulseshaping):
 * every row of E (nmodes, L) through the rational polyphase FIR
 *     out[k] = gain * sum_m h[k down + (ntaps - 1) / 2 - m up] E[m],   k = 0 .. Lout - 1,   E zero outside the row,
 * h: ntaps real taps in HOST memory (double; cast to the signal's precision, accumulation in that precision).  gain = up is scipy's
 * resample_poly(window = h), gain = 1 zero insertion + fftconvolve(.., 'same') + decimation, up = down = 1 a 'same' convolution.
 * 1 <= up, down <= 64; 1 <= ntaps <= 8191; Lout <= ceil(L up / down); out (nmodes, Lout) must not alias E.  The phase-major table is
 * uploaded once per distinct (taps, up, precision).  Deterministic (no atomics). */
int qh_resample_c64(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out);
int qh_resample_c128(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out);
int qh_resample_c64_dev(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out);
int qh_resample_c128_dev(const void *E, int nmodes, int64_t L, const double *h, int ntaps, int up, int down, double gain, int64_t Lout, void *out);
/* Per-row moments of E (nmodes, L) on the device: mom[3 row + {0, 1, 2}] = mean re, mean im, mean |.|^2, accumulated in double in a fixed
 * order; mom is DEVICE memory (3 nmodes doubles).  qh_center_scale: X <- (X - mean) sqrt(P / (mean |X|^2 - |mean|^2)) in place, the moments
 * of X read from device memory; P = mom_in[3 row + 2] (the moments of another array, e.g. the resampler's input: the reference's
 * renormalise=True), or `target` when mom_in is NULL.  Enqueue only: nothing is read back. */
int qh_row_moments_c64_dev(const void *E, int nmodes, int64_t L, double *mom);
int qh_row_moments_c128_dev(const void *E, int nmodes, int64_t L, double *mom);
int qh_center_scale_c64_dev(void *X, int nmodes, int64_t L, const double *mom, const double *mom_in, double target);
int qh_center_scale_c128_dev(void *X, int nmodes, int64_t L, const double *mom, const double *mom_in, double target);

/* ---- select_angles: out[i] = angles[(p > 1 ? i : 0), idx[i]] ;  idx int64 (L,) ------------------------------- */
int qh_select_angles_f32(const void *angles, int64_t p, int A, const int64_t *idx, int64_t L, void *out);
int qh_select_angles_f64(const void *angles, int64_t p, int A, const int64_t *idx, int64_t L, void *out);

/* ---- make_decision: nearest alphabet point, |distance| (not squared) and index (first minimum) --------------- */
int qh_make_decision_c64(const void *E, int64_t L, const void *symbols, int M, void *det, void *dist, int32_t *idx);
int qh_make_decision_c128(const void *E, int64_t L, const void *symbols, int M, void *det, void *dist, int32_t *idx);
int qh_make_decision_c64_dev(const void *E, int64_t L, const void *symbols, int M, void *det, void *dist, int32_t *idx);
int qh_make_decision_c128_dev(const void *E, int64_t L, const void *symbols, int M, void *det, void *dist, int32_t *idx);

/* ---- measurement helpers ---------------------------------------------------------------------------------------
 * symbol errors of decided indices against a reference index sequence with a lag: count(idx_rx[i] != idx_tx[i - lag]) over the i < n
 * with 0 <= i - lag < ntx.  idx_rx (n,), idx_tx (ntx,) and count_dev (one unsigned 64-bit counter) live in HBM.  The count is ADDED to
 * *count_dev, which is never cleared here: the caller zeroes it, and may accumulate several calls in it; n <= 0 leaves it alone.  The
 * launch is asynchronous on the library stream.  A NULL pointer or ntx < 0 returns QH_ERR_ARG before anything is launched. */
int qh_count_errors_dev(const int32_t *idx_rx, const int32_t *idx_tx, int64_t n, int64_t lag, int64_t ntx,
                        unsigned long long *count_dev);

/* Form of the exact trainer for subsequent calls: 0 automatic (default), 1 direct, 2 look-ahead, 3 block-iterative (the same
 * switch as qh_set_form("trainer", ...)).  All forms give the
 * reference's results up to the order of floating-point additions; a form that cannot take a call falls through. */
int qh_set_trainer(int form);
/* Production knobs (ABI 8; rounds 1-4 read environment variables in the launch paths).  The environment variables of the same meaning
 * (QAMPY_HIP_RESERVED_CUS, QAMPY_HIP_GRAM_BUDGET_GB) are read ONCE, as the initial value, when the value is first needed.
 *   qh_set_reserved_cus(n)     compute units library stream 2 stays off (default 32; 0: none); applies to streams created afterwards - call it before a
 *                              thread's first library call, or after qh_thread_release
 *   qh_set_gram_budget_gb(gb)  scratch the Gram tables of one call may take (default 160 of the 288 GB); longer captures / larger banks train in time chunks
 *   qh_set_default_tier(tier, tol)
 *                              what the DROP-IN host-array trainers (qh_train_equaliser_c64 / _c128 - the entry points a binding of the reference's
 *                              `train_equaliser` export calls) run: 0 = tier a, the exact sequential recurrence (default); 1 = tier b, the
 *                              same recurrence solved in parallel in time to `tol` (0 = 1e-3; SURVEY.md 8c's complex64 bar is 1e-4), total: a call no
 *                              parallel-in-time solver exists for, or one the passes do not certify, runs in the exact form inside the call.
 *                              qh_last_pit_report: the device's report of the calling thread's most recent such solve. */
int qh_set_pit_timing(int mode);      /* which relaxation passes of a tier-b sweep get HIP events (qh_pit_last_timing): 0 none, 1 pass 1 of every sweep (default: an event
                                        * idles the stream for ~5.6 us), 2 every pass (bench.py's roofline run) */
int qh_set_reserved_cus(int n);
int qh_set_gram_budget_gb(double gb);
int qh_get_gram_budget_gb(double *gb);
int qh_set_default_tier(int tier, double tol);
int qh_get_default_tier(int *tier, double *tol);
/* Test hooks (ABI 10; rounds 1-5 read environment variables in the launch paths): each forces a kernel form the automatic choice would not take at
 * that size, none selects a different algorithm, every one is exercised through this C ABI by the -m gpu tests named.  The launch paths read ONE table
 * of atomics; the environment variables of the same meaning (QAMPY_HIP_TRAINER, QAMPY_HIP_PIT_FORM, QAMPY_HIP_SEG_LANES, QAMPY_HIP_PIT_PROBE,
 * QAMPY_HIP_BPS, QAMPY_HIP_PIT_TAIL) are read ONCE, when the library is loaded, as the table's initial values.
 *   key          values                                        what
 *   "trainer"    auto | direct | lookahead | iterative          form of the exact trainer, like qh_set_trainer (tests/test_gpu_parity.py)
 *   "pit_form"   auto | segment | block                         parallel in time: throughput / latency form of the passes (tests/test_gpu_pit.py)
 *   "seg_lanes"  0 | 8 | 16                                     throughput form: lanes per chain (tests/test_gpu_pit.py)
 *   "pit_probe"  0 | 1                                          complex64: the complex128 analysis of a pass (probe of the capture) (tests/test_gpu_pit.py)
 *   "bps"        auto | tile | lds                              phase search: tile kernel for complex64 / streaming kernel with the LDS ring only (no
 *                                                               register-ring kernel) (tests/test_gpu_parity.py)
 *   "pit_tail"   auto | split                                   parallel in time, eigen-space analysis: auto ends a pass with ONE launch - estimate, decision and
 *                                                               the back product for the next pass - where the sweep allows it (throughput form, fixed
 *                                                               step, whole capture); split keeps the two launches every other sweep uses.  Same
 *                                                               operations on the same values either way (tests/test_gpu_pit_tail.py)
 * qh_set_form returns QH_ERR_ARG for an unknown key or value; a NULL or empty value resets the key to automatic.  qh_get_form returns QH_ERR_ARG
 * for an unknown key or a NULL value. */
int qh_set_form(const char *key, const char *value);
int qh_get_form(const char *key, int *value);

/* ---- parallel-in-time training ("tier B": opt-in, NOT the reference's order of evaluation) -----------
 * The sweep of TrSyms steps is cut into S contiguous segments that are trained CONCURRENTLY with the exact kernels
 * (segments = the channels of a batch that happen to be adjacent in one capture) and made consistent by waveform
 * relaxation: in pass p segment s starts from the taps segment s-1 ended with in pass p-1 (segment 0 always from the start
 * taps).  The map is triangular in s, its only fixed point is the sequential recurrence, reached exactly after S passes;
 * in practice the LMS recursion forgets its start within a few 1/(mu lambda) steps and the passes stop as soon as the
 * boundary DEFECT - the relative rms difference, on a probe window of the capture, between the outputs of the taps a
 * segment started from and the taps its left neighbour ended with, modulo the symmetry of the error function (common
 * phase for cma / rde, quarter turns for the square-grid functions) - is below `tol` for every boundary.  Everything is
 * decided on the device (skip flags): the call only enqueues, nothing synchronises.
 *   acquire != 0 (cold start, e.g. centre-spike taps): a sequential "acquisition" first trains a prefix of the capture with
 *     a gear-shifted step size mu_acq = clamp(gear * mu, mu, acq_bound / (nmodes ntaps <|x|^2>)) in chunks until the mean
 *     squared error stops improving (or acq_max steps).  The acquired taps SEED the start taps of segments 1 .. S-1; segment 0
 *     starts from the caller's taps (start = 0, the default), so the fixed point of the passes is the reference's recurrence from
 *     the caller's taps - the cold-start trajectory itself.  start = 1 is the round-2 behaviour: segment 0 starts from the
 *     acquired taps too, i.e. the result is the recurrence WARM-STARTED from them (one or two passes fewer, taps of the weakly
 *     excited directions ~1e-2 away from the cold-start result).
 *   Stop rule (`tol`): with the coarse correction on, the passes stop when the ESTIMATED DEVIATION of the pass's trajectory from
 *     the sequential recurrence - relative rms deviation of the equaliser OUTPUT, worst segment - is below tol.  The estimate is
 *     the first-order solution of the error equation E[s+1] = F'_s E[s] + d[s+1] (d the boundary defects of the pass, F'_s the
 *     segment Jacobian replaced by its linearised model J), measured in output power: sum_k lambda_k |E~_k[s]|^2 / <|y|^2> in the
 *     eigenbasis of the input covariance - the same scan that forms the next correction; the rule takes its rms over all segments
 *     and modes (times dev_safety, default 1: measured against the exact path the estimate is within a factor 1.5 of the rms
 *     deviation of the error trace) and additionally holds the worst segment below 3 tol and the estimated relative deviation of
 *     the taps themselves (unweighted norm of the same vectors, rms over the segments: the weakly excited directions count fully)
 *     below 2 tol.  Measured against the exact path the FINAL taps sit at the worst-segment value of that estimate (deviation_taps_worst,
 *     up to 1.6 x the rms: deviations of the weakly excited directions accumulate along the sweep), i.e. within 3 tol.
 *     Without the correction (nmodes * ntaps > 128, or switched off) the round-2 rule applies: largest boundary
 *     defect x a segment-length factor below tol.
 *   phase_seed: for the phase-sensitive functions (mcma, mrde, sbd, mddma, dd) the pass-0 start taps of segment s are the
 *     start taps rotated by an unwrapped 4th-power phase estimate of their output at the head of the segment, so that
 *     every segment starts phase-locked however far the carrier has drifted (-1: by method, 0 off, 1 on).
 *   correction: plain relaxation hands information on by ONE segment per pass, which is fine for the tap directions the
 *     signal excites (they forget within a segment) but not for the weakly excited ones (out-of-band directions, time
 *     constants 1/(mu g lambda) of millions of steps), whose state depends on the whole history.  Between the passes
 *     the boundary defects d[s] are therefore propagated through the LINEARISED segment map J = exp(-mu g T Rc), Rc the
 *     input covariance <conj(x) x^T> and g the mean gain of the error function: D[s+1] = d[s+1] + J D[s] (in the
 *     eigenbasis of Rc: one scalar first-order recurrence per direction, run as a parallel scan), start taps += D.  With J = 0 this is plain relaxation; J only preconditions the
 *     iteration - at the fixed point all defects vanish and the result is the sequential recurrence either way.
 * Fixed step, or the adaptive step through qh_pit_opts.adaptive (one output mode per call, see there); no data-aided methods.
 * EVERY call returns the reference's result: a sweep that is not certified is redone in the exact form inside the call
 * (qh_pit_opts.exact_redo_off, qh_pit_report.converged = 2).  gram: table from qh_gram_build_*_dev for this (E, os, ntaps,
 * TrSyms), or NULL.  report_dev: device memory for one qh_pit_report (read it after qh_sync), or NULL. */
#define QH_PIT_MAXPASS 24
#define QH_PIT_MAXCHUNK 32
typedef struct qh_pit_opts {
    int32_t segments;       /* 0 = automatic: segments of about 0.2 / mu (warm) or 0.4 / mu (cold start) steps, qh_pit_auto_segments */
    int32_t max_passes;     /* 0 = 16 (at most QH_PIT_MAXPASS) */
    int32_t acquire;        /* 0 warm start, 1 cold start: gear-shifted sequential acquisition first */
    int32_t phase_seed;     /* -1 by method, 0 off, 1 on */
    double tol;             /* 0 = 1e-3: accepted estimated rms deviation of the equaliser output from the sequential recurrence, relative to the
                             * output rms (see "Stop rule"); without the coarse correction: largest boundary defect accepted */
    double gear;            /* 0 = 8 */
    double acq_bound;       /* 0 = 0.08 */
    double acq_plateau;     /* 0 = 0.8: a chunk whose mean |err|^2 exceeds this fraction of the previous one's ends the acquisition */
    int64_t acq_chunk;      /* 0 = automatic: 2 / mu_acq steps (mu_acq = the gear-shifted step size) rounded to the nearest power of two, 256 .. 4096 */
    int64_t acq_max;        /* 0 = two chunks (at most TrSyms / 2 steps) */
    int32_t correction;     /* -1 / 1: linearised coarse correction between the passes (see below), 0: plain relaxation - every pass up to
                             * max_passes runs unless the tolerance is met (no "nothing gained over two passes" stop: S passes over S segments are
                             * the sequential recurrence, and the boundary defects need not fall before the last one) */
    int32_t head_steps;     /* fixed step: > 0 - the first head_steps steps of every sweep run in the EXACT form, the segments cover the rest; 0: none, unless
                             * the passes stall on the start of the sweep (see head_auto_off) (ABI 6) */
    void *basis;            /* NULL, or the eigenbasis of this capture's input covariance from qh_pit_basis_*_dev (device memory) */
    double corr_beta;       /* extra damping of the well-excited directions in the coarse map, exp(-a (1 + beta a)); < 0: by method */
    /* One capture over several processes / GPUs (optional; every process holds the whole capture and makes the same call):
     * this process trains segments [seg_first, seg_first + seg_count) only (exchange == NULL: all of them; with an exchange
     * callback seg_count = 0 means "none": the process still takes part in every exchange); after the training
     * launch of every pass the library zeroes the end taps of the segments it does not own, synchronises its stream (unless
     * exchange_on_stream) and calls
     * exchange(exchange_user, taps, bytes) - the caller sums the buffers of all processes in place (an all-reduce: RCCL over
     * xGMI) and returns 0 - after which every process evaluates the (cheap) boundary defects and the coarse correction on
     * identical data and takes identical decisions.  Error traces are written for the owned segments only. */
    int32_t seg_first, seg_count;
    int (*exchange)(void *user, void *taps_dev, size_t bytes);
    void *exchange_user;
    int32_t start;          /* 0: segment 0 starts from the caller's taps (fixed point = the reference's recurrence); 1: from the acquired taps */
    int32_t exchange_on_stream; /* != 0: `exchange` only ENQUEUES the all-reduce on the library stream (RCCL with qh_stream_handle): the library
                             * does not synchronise around it and enqueues the next pass ahead as in the single-process case */
    double dev_safety;      /* 0 = 1: factor on the deviation estimate in the stop rule */
    int32_t adaptive;       /* != 0: the step size adapts (adapt_step); ONE output mode per call (nsel = 1), one sweep, complex64, cma / mcma / sbd /
                             * mddma; mu is in/out like in the exact entry points.  The first 16384 steps run in the exact form, the sweep is held to
                             * tol / 3 with up to 24 passes (damped corrections); one that is not certified is redone in the exact form
                             * (report: converged = 2) (ABI 4) */
    int32_t exact_redo_off; /* 0 (default): a sweep the passes do not certify (estimate above tol when they stop, pass budget used up, no coarse
                             * model) is redone in the EXACT form from the taps the call started with, inside the call - every call returns the
                             * reference's result; report: converged = 2.  != 0: the uncertified result stays (converged = 0) (ABI 5) */
    int32_t head_auto_off;  /* 0 (default): a sweep whose passes stall with the estimated deviation confined to the first quarter of the segments (a
                             * non-linear transient at the start of the stage: e.g. a decision-directed stage pulling in from taps locked to another
                             * carrier phase) is repeated with that stretch as an exact head - sequential there, parallel in time after it - before the
                             * whole call is given to the exact form; != 0: off (ABI 6) */
    int32_t acq_anneal;     /* acquisition: 0 (default) the second and later chunks run at half the step of the one before, never below 2 mu; > 0: never
                             * below acq_anneal x mu; < 0: every chunk at the gear-shifted step (rounds 2-3) (ABI 6) */
    double mu_hint;         /* fixed step: the caller's HOST copy of *mu (> 0), so that the call does not have to read it back; with it - and acq_chunk
                             * given when acquire != 0 - the call enqueues its whole prologue without a host synchronisation (0: read back) (ABI 7) */
    void *prepared;         /* cold start (acquire != 0): NULL, or the device buffer a qh_pit_prepare_*_dev call for THIS capture, these start taps, this step
                             * size and method filled: the acquisition has run already (beside the previous capture's training, on another stream) -
                             * the call adopts its taps and report fields instead of running it.  The caller orders the two (qh_stream_wait_event). (ABI 8) */
    void (*on_pass0)(void *user);   /* NULL, or a function the call invokes ONCE, on the calling thread, right after it has enqueued the first relaxation pass: the
                             * place to enqueue work for OTHER library streams (the previous capture's phase search, the next capture's preparation) whose
                             * launches would otherwise sit in front of this sweep's; it must leave the current library stream as it found it (ABI 8) */
    void *on_pass0_user;
    void (*on_pass)(void *user, int sweep, int pass);   /* NULL, or a function the call invokes on the calling thread right BEFORE it enqueues the trainer launch of
                             * relaxation pass `pass` of sweep `sweep`: the place to enqueue chip-wide work of other library streams behind an event recorded
                             * here - it then starts together with the trainer and runs beside it (qh_bps_recover_part_*_dev: a part of the phase search small
                             * enough to be one wave per SIMD costs the pass 0-3 %), not in the ~70 us of analysis behind the trainer, which are the critical
                             * path.  A pass enqueued ahead of the decision that ends the sweep still calls it (its launches do nothing).  It must leave the
                             * current library stream as it found it (ABI 9) */
    void *on_pass_user;
} qh_pit_opts;
typedef struct qh_pit_report {
    int32_t segments, passes, converged, acq_chunks;
    int64_t seg_len, acq_steps;
    double mu, mu_acq, power, tol;
    double defect[QH_PIT_MAXPASS];      /* largest boundary defect after pass p of the last sweep; -1 = pass not run */
    double acq_err[QH_PIT_MAXCHUNK];    /* mean |err|^2 of the acquisition chunks */
    double gain, out_power;             /* linearised error-function gain g and mean output power used by the correction */
    int32_t acq_done, done, diverged, corr_on;   /* device-side flags */
    double result_change[QH_PIT_MAXPASS]; /* how far the sweep's RESULT (end taps of the last segment) moved from pass p-1 to pass p, as the relative
                                            rms difference of the two outputs on the last 128 steps (modulo the error function's symmetry);
                                            pass 0: against the start taps; -1 = not run */
    double deviation[QH_PIT_MAXPASS];   /* estimated relative rms output deviation of pass p's trajectory from the sequential recurrence (worst
                                            segment, without the safety factor); -1 = not available (no coarse correction) */
    double deviation_rms[QH_PIT_MAXPASS]; /* the same estimate as an rms over all segments and modes */
    double deviation_taps[QH_PIT_MAXPASS]; /* estimated deviation of the TAPS from the sequential recurrence's: |D[s]| / |w|, rms over segments and modes */
    double deviation_taps_worst[QH_PIT_MAXPASS]; /* ... of the worst segment */
} qh_pit_report;
int qh_pit_auto_segments(int64_t TrSyms, double mu, int nsel, int cold, int *segments);   /* cold: the sweep starts from unconverged taps (acquire) */
/* Eigenbasis of the input covariance <conj(x) x^T> of the training windows of a capture, for the coarse correction: depends
 * on (E, os, ntaps, TrSyms) only, so one build serves every stage and sweep over the same capture.  basis: device memory of
 * qh_pit_basis_bytes(nmodes*ntaps) bytes.  nmodes*ntaps <= 128.  overlap != 0: built on the library's other stream while the
 * current stream goes on (the trainer waits for it before its first correction; qh_sync waits for both streams). */
int qh_pit_basis_bytes(int ntot, size_t *bytes);
int qh_pit_basis_c64_dev(const void *E, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void *basis, int overlap);
int qh_pit_basis_c128_dev(const void *E, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void *basis, int overlap);
/* kernel time (HIP events on the library stream) of the trainer launches of the most recent qh_train_equaliser_*_pit_dev call:
 * the timed relaxation passes in order (all sweeps) and the sum of the acquisition chunks.  An event idles the stream for ~5.6 us,
 * so by default ONE pass per sweep is timed (pass 1); qh_set_pit_timing(2) times every pass. */
int qh_pit_last_timing(float *pass_ms, int max_passes, int *npass, float *acq_ms);
/* Which kernel form took the relaxation passes of the calling thread's most recent qh_train_equaliser_*_pit_dev call (read-only, host-side
 * values; tests pin a kernel instantiation with it).  form: 0 the exact form only (no passes were launched), 1 segment (throughput form),
 * 2 block-iterative, 3 look-ahead, 4 direct.  For the segment form: lanes per chain (16 / 8), taps per lane, padding taps in the last lane
 * of an input mode, size of the partition / slicer table the kernel was instantiated for, adaptive-step kernel (0 / 1); zeros otherwise.
 * (0 for the error functions whose kernels carry no table: cma, sgncma, cma2, mcma).  A call that falls back to the exact form after its
 * passes keeps the passes' values; a call refused on its arguments leaves zeros; a process of a split capture that owns no segment
 * reports form 1 and no layout.  Any pointer may be NULL.  form = 0 before any call. */
int qh_pit_last_launch(int *form, int *lanes, int *tpl, int *rag, int *npart, int *adaptive);
/* The sequential part of a COLD sweep ahead of time (ABI 8): the gear-shifted acquisition of a capture depends on the capture, the start taps, the step
 * size and the error function only - not on anything the previous capture's training produces - so a receiver that is handed capture after capture runs
 * it for capture k + 1 on another library stream while capture k trains (pipeline.ResidentReceiver.run(prefetch=True)), and hands the result to the
 * training call through qh_pit_opts.prepared.  Same kernels on the same data as the acquisition inside the call: bit-identical results.
 * opts: as for the training call (segments, mu_hint and acq_chunk must be given - the call never synchronises); prep: device memory of
 * qh_pit_prepare_bytes(...) bytes.  Returns QH_ERR_ARG with "not preparable" for a sweep whose acquisition cannot run ahead (decision-directed or
 * adaptive stages, latency-form passes): the caller then simply does not pass `prepared`. */
int qh_pit_prepare_bytes(int nmodes, int ntaps, int64_t acq_steps, size_t elem_bytes, size_t *bytes);
int qh_pit_prepare_c64_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int os, const float *mu_dev, const void *wx0, int ntaps,
                           const int64_t *modes, int nsel, const void *symbols, int64_t nsy, int method, const qh_pit_opts *opts, void *prep, size_t prep_bytes);
int qh_last_pit_report(qh_pit_report *out);      /* host copy of the report of the calling thread's most recent host-array solve through tier b (qh_set_default_tier) */
int qh_train_equaliser_c64_pit_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, float *mu_dev,
                                   void *wx, int ntaps, const int64_t *modes, int nsel, const void *symbols, int64_t nsy,
                                   int method, void *err, int zero_err, const void *gram, const qh_pit_opts *opts,
                                   void *report_dev);
int qh_train_equaliser_c128_pit_dev(const void *E, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os, double *mu_dev,
                                    void *wx, int ntaps, const int64_t *modes, int nsel, const void *symbols, int64_t nsy,
                                    int method, void *err, int zero_err, const void *gram, const qh_pit_opts *opts,
                                    void *report_dev);

/* ---- channel bank: nch independent captures of identical shape processed together -------------------------------
 * (SURVEY.md 8e "within a GPU": one exact training chain occupies one workgroup, so a GPU holds hundreds of channels).
 * All arrays carry a leading channel dimension and are contiguous: E (nch, nmodes, L), wx (nch, nmodes, nmodes, ntaps),
 * err (nch, nmodes, TrSyms*Niter), mu_dev (nch,), gram = nch tables from qh_gram_build_*_batch_dev (or NULL: built
 * internally); symbols and modes are shared.  Semantics per channel: exactly qh_train_equaliser_*_dev. */
int qh_gram_build_c64_batch_dev(const void *E, int nch, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void **gram);
int qh_gram_build_c128_batch_dev(const void *E, int nch, int nmodes, int64_t L, int os, int ntaps, int64_t TrSyms, void **gram);
int qh_train_equaliser_c64_batch_dev(const void *E, int nch, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os,
                                     float *mu_dev, void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive,
                                     const void *symbols, int64_t nsy, int method, void *err, int zero_err, const void *gram);
int qh_train_equaliser_c128_batch_dev(const void *E, int nch, int nmodes, int64_t L, int64_t TrSyms, int Niter, int os,
                                      double *mu_dev, void *wx, int ntaps, const int64_t *modes, int nsel, int adaptive,
                                      const void *symbols, int64_t nsy, int method, void *err, int zero_err, const void *gram);

/* On-device SER harness (reference: cal_ser core/signals.py:295-335 = sync_and_adjust /
 * find_sequence_offset_complex core/ber_functions.py:33-160 + make_decision + compare).  E: one recovered row (N,) in
 * HBM; idx_tx: decided indices of the transmitted symbols (nmodes, ntx) int32 in HBM (qh_make_decision_*_dev); symbols
 * (M,) in HBM.  Bounded search over tx mode x quadrant rotation x lag in [-maxlag, maxlag] on a `window` of decided
 * symbols from the middle of the run, then errors over [trim, N - trim).  result (HOST, 7 x int64): errors, compared,
 * tx mode, rotation k (row was multiplied by j^k), lag (rx[i] <-> tx[i - lag]), matches in the window, window length.
 * Window: W = window > 0 ? window : 4096, then min(W, N - 2 trim), starting at trim + (N - 2 trim - W) / 2 (integer division).  The
 * winner is the FIRST maximum of the match counts in (tx mode, rotation, lag) order, lags ascending from -maxlag.  Only symbols with
 * 0 <= i - lag < ntx are matched or compared; a label outside [0, M) never matches.  1 <= nmodes <= 16, M >= 1, 0 <= maxlag <= 4096,
 * trim >= 0, 2 trim < N; bad sizes and NULL pointers return QH_ERR_ARG before anything is launched and leave result untouched. */
int qh_ser_c64_dev(const void *E, int64_t N, const int32_t *idx_tx, int nmodes, int64_t ntx, const void *symbols, int M,
                   int maxlag, int64_t window, int64_t trim, int64_t *result);
int qh_ser_c128_dev(const void *E, int64_t N, const int32_t *idx_tx, int nmodes, int64_t ntx, const void *symbols, int M,
                    int maxlag, int64_t window, int64_t trim, int64_t *result);

/* ---- signal-quality metrics (metrics.hip).  Reference: the last `#pythran export`s of qampy/core/pythran_dsp.py that
 * qampy/core/signal_quality.py:27-29 binds - soft_l_value_demapper (:87-104), soft_l_value_demapper_minmax (:106-131),
 * estimate_snr (:244-286), cal_mi_mc (:289-300), cal_mi_mc_fast (:303-313) - and the metric methods of qampy/signals.py:295-560.
 * `alphabet` (M,) is the constellation in coded order: point g carries Gray label g, bit k of it (MSB first) is
 * (g >> (nbits - 1 - k)) & 1, so no bit table is passed (the python layer inverts the reference's bits_map).  M = 2^nbits,
 * nbits 1..10, for everything that works on bits; M <= 1024 for the rest.  Sums are reduced in double in a fixed order:
 * repeated calls give bit-identical results.  Bad sizes, an nbits other than log2 M, 2 trim >= N and an alignment without
 * overlap return QH_ERR_ARG before anything is launched. */
/* L (N, nbits) float64: log-likelihood ratios ln P(bit = 1) / P(bit = 0) at linear `snr`; complex64 input is evaluated in
 * float with each (bit, side) sum shifted by its own minimum distance, so L stays finite far beyond fp32's exp range. */
int qh_soft_l_value_demapper_c64(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L);
int qh_soft_l_value_demapper_c128(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L);
int qh_soft_l_value_demapper_minmax_c64(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L);
int qh_soft_l_value_demapper_minmax_c128(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, double *L);
int qh_soft_l_value_demapper_c64_dev(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L);
int qh_soft_l_value_demapper_c128_dev(const void *rx, int64_t N, int nbits, double snr, const void *alphabet, int M, int minmax, double *L);
/* estimate_snr: result (HOST, 3 doubles) = linear snr, S0, N0.  Classes are the alphabet points tx equals exactly; ntx == N.
 * An empty class gives NaN (np.mean of an empty selection), as in the reference. */
int qh_estimate_snr_c64(const void *rx, int64_t N, const void *tx, int64_t ntx, const void *alphabet, int M, double *result);
int qh_estimate_snr_c128(const void *rx, int64_t N, const void *tx, int64_t ntx, const void *alphabet, int M, double *result);
/* cal_mi_mc (noise (L,)) and cal_mi_mc_fast (x, tx (L,)): *mi (HOST) in bits per symbol. */
int qh_cal_mi_mc_c64(const void *noise, int64_t L, const void *alphabet, int M, double N0, double *mi);
int qh_cal_mi_mc_c128(const void *noise, int64_t L, const void *alphabet, int M, double N0, double *mi);
int qh_cal_mi_mc_fast_c64(const void *x, const void *tx, int64_t L, const void *alphabet, int M, double N0, double *mi);
int qh_cal_mi_mc_fast_c128(const void *x, const void *tx, int64_t L, const void *alphabet, int M, double N0, double *mi);
/* Device-resident forms on one row E (N,) in HBM against idx_tx (ntx,) int32 in HBM (one transmitted mode, e.g. a row of
 * qh_make_decision_*_dev's output), aligned like qh_ser_*_dev's result: E[i] * j^rot is compared with alphabet[idx_tx[i - lag]]
 * for i in [trim, N - trim) with 0 <= i - lag < ntx (labels outside [0, M) are skipped).  alphabet (M,) in HBM.
 * qh_estimate_snr_*_dev: result (HOST, 3 doubles) snr, S0, N0 over that overlap.
 * qh_metrics_*_dev: one pass, no LLR stored; decisions as qh_ser_*_dev.  counts (HOST, 3 x int64): symbol errors, bit errors,
 * compared symbols.  sums (HOST, 2 + nbits doubles): sum |t - r|^2; sum log2 sum_j exp(-(|r - s_j|^2 - |r - t|^2) snr) (the fast
 * MI with N0 = 1 / snr); per bit k sum log2(1 + exp((-1)^b L_k)) with exact (minmax = 0) or max-log (minmax = 1) LLRs at `snr`. */
int qh_estimate_snr_c64_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                            int64_t trim, double *result);
int qh_estimate_snr_c128_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                             int64_t trim, double *result);
int qh_metrics_c64_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                       int64_t trim, double snr, int minmax, int64_t *counts, double *sums);
int qh_metrics_c128_dev(const void *E, int64_t N, const int32_t *idx_tx, int64_t ntx, const void *alphabet, int M, int rot, int64_t lag,
                        int64_t trim, double snr, int minmax, int64_t *counts, double *sums);

/* On-device synthesis of an impaired capture (the reference builds its test signals with signals.py,
 * core/resample.py:73-126 and core/impairments.py:94-233): random Gray-labelled M-QAM symbols (Philox, keyed by seed /
 * mode / symbol index), root-raised-cosine shaping at `os` samples per symbol, optional Wiener phase noise (phase_var =
 * 2 pi linewidth / fs per sample), first-order PMD (theta, DGD in samples; 2 modes) and AWGN at snr_db (reference
 * convention sigma = 10^(-snr/20) sqrt(os)).  Outputs in HBM: E (nmodes, nsym*os) complex64, symbols (nmodes, nsym)
 * complex64, idx_tx (nmodes, nsym) int32 (index into alphabet).  alphabet (M,) complex64 in HBM. */
int qh_synth_capture_c64_dev(void *E, void *symbols, int32_t *idx_tx, const void *alphabet, int M, int nmodes, int64_t nsym,
                             int os, double beta, double snr_db, int have_snr, double theta, double dgd_samples, int have_pmd,
                             double phase_var, uint64_t seed);

/* ---- whole-row transforms (csrc/fft.hip): DFT (inverse != 0: inverse DFT, with numpy's 1 / L) along the last axis of E (nmodes, L) into
 * out (nmodes, L); out may be E itself.  L: a power of two from 2^8 to 2^24, or any other length from 2 to 2^23 (Bluestein); anything else:
 * QH_ERR_ARG before a launch.  Device pointers, nothing read back, enqueued on the current stream; a repeated call is bit-identical. */
int qh_fft_c64_dev(const void *E, int nmodes, int64_t L, int inverse, void *out);
int qh_fft_c128_dev(const void *E, int nmodes, int64_t L, int inverse, void *out);
/* out = ifft(H . fft(E)) of every row, same lengths, H (L bins in numpy's fftfreq order) formed on the device in double.  kind:
 *   1 brick wall  keep the bins whose position after fftshift lies in [i0, i1) (core/filter.py:28-49 pre_filter)
 *   2 band        keep |k p0 - p1| < p2, k the signed bin number: p0 = 1 / (L d) of fftfreq(L, d), p1 the centre, p2 half the width
 *   3 two rails   Hi = exp(-2 pi i p1 f), Hq = exp(-2 pi i p2 f), f = k p0: out = Re(D_p1{Re E}) + i Re(D_p2{Im E}), one transform pair
 *   4 delay       H = exp(-2 pi i p1 f), f = k p0
 *   5 / 6         H: a device table of L values, real in the field's real type / complex in the field's type
 * out may be E itself. */
int qh_spectral_filter_c64_dev(const void *E, int nmodes, int64_t L, int kind, double p0, double p1, double p2, int64_t i0, int64_t i1,
                               const void *H, void *out);
int qh_spectral_filter_c128_dev(const void *E, int nmodes, int64_t L, int kind, double p0, double p1, double p2, int64_t i0, int64_t i1,
                                const void *H, void *out);
/* ---- IQ conditioning (csrc/iq.hip; qampy/core/analog_frontend.py).  mom (nmodes, 10) doubles: sum I, sum Q, sum I^2, sum Q^2, sum I Q of every
 * row of E (nmodes, L) over all samples, then the same five over every os-th sample; two launches, bit-reproducible. */
int qh_iq_moments_c64_dev(const void *E, int nmodes, int64_t L, int os, double *mom);
int qh_iq_moments_c128_dev(const void *E, int nmodes, int64_t L, int os, double *mom);
/* coef (nmodes, 6) doubles (a00, a01, a10, a11, b0, b1) of y = A (I, Q)^T + b from mom.  kind 0: orthonormalize_signal(E, os), row by row;
 * 1: comp_IQ_inbalance, moments pooled over all rows; 2: the centring of comp_IQ_inbalance alone.  Device pointers, one workgroup. */
int qh_iq_coeffs_dev(const double *mom, int nmodes, int64_t L, int os, int kind, double *coef);
/* out = A (Re E, Im E)^T + b per row, evaluated in double; out may be E. */
int qh_iq_affine_c64_dev(const void *E, int nmodes, int64_t L, const double *coef, void *out);
int qh_iq_affine_c128_dev(const void *E, int nmodes, int64_t L, const double *coef, void *out);

/* ---- synchronisation of a received row with a transmitted one (csrc/sync.hip; qampy/core/ber_functions.py:33-160).  Device pointers unless
 * said otherwise, enqueued on the current stream, nothing read back, no atomics: a repeated call is bit-identical.
 * cc (nx_rows, nx + ny - 1) = fftconvolve(x, conj(y)[::-1], "full") of every row of x (nx_rows, nx) with the one row y (ny,): the peak of |cc|
 * at index k says y lies k - (ny - 1) samples into x.  Three power-of-two transforms of size P >= max(nx + ny - 1, 2^8); nx < 1, ny < 1 or
 * nx + ny - 1 > 2^24: QH_ERR_ARG before a launch.  The work buffers are cached: a call at a shape seen before allocates nothing. */
int qh_xcorr_c64_dev(const void *x, int nx_rows, int64_t nx, const void *y, int64_t ny, void *cc);
int qh_xcorr_c128_dev(const void *x, int nx_rows, int64_t nx, const void *y, int64_t ny, void *cc);
/* res (rows, 6) doubles per row of cc (rows, n): the index of the first maximum of |cc| (np.argmax: ties to the lower index, a NaN before any
 * number), max Re, max Im, max -Re, max -Im (NaN if the row holds one, as np.max) and |cc| at that index, compared in the field's real type.
 * Two launches: one partial per tile, one workgroup over the partials. */
int qh_xcorr_peak_c64_dev(const void *cc, int rows, int64_t n, double *res);
int qh_xcorr_peak_c128_dev(const void *cc, int rows, int64_t n, double *res);
/* out[i] = 1j^turns src[(i - offset) mod nsrc], i in [0, nout): the roll, roll-and-cut and periodic extension of sync_and_adjust in one
 * formula; the rotation is exact (a swap and a sign); offset may be negative; out must not be src.  The i32 form moves label rows. */
int qh_cyclic_gather_c64_dev(const void *src, int64_t nsrc, int64_t offset, int turns, int64_t nout, void *out);
int qh_cyclic_gather_c128_dev(const void *src, int64_t nsrc, int64_t offset, int turns, int64_t nout, void *out);
int qh_cyclic_gather_i32_dev(const int32_t *src, int64_t nsrc, int64_t offset, int64_t nout, int32_t *out);
/* out[i] = alphabet[idx[i]], i in [0, n); a label outside [0, M) gives 0. */
int qh_labels_to_symbols_c64_dev(const int32_t *idx, int64_t n, const void *alphabet, int M, void *out);
int qh_labels_to_symbols_c128_dev(const int32_t *idx, int64_t n, const void *alphabet, int M, void *out);

/* ---- bit source and Gray mapper (csrc/source.hip; qampy/core/prbs.py, qampy/signals.py:89-137, :678-731).  Device pointers, enqueued on the
 * current stream, nothing read back, no atomics and no scratch: a repeated call is bit-identical.  Integer work and table look-ups only: the
 * results are the reference's bit for bit.  Bits are one byte each, 0 or 1 (numpy's bool layout).
 * bits[i] = bit start + i of the PRBS of `order` (7, 15, 23 or 31), i in [0, n), complemented if invert != 0.  kind 0: external XOR
 * (pythran_dsp.prbs_ext with the taps of make_prbs_extXOR); kind 1: internal XOR (pythran_dsp.prbs_int(seed, mask, order, n) with the masks of
 * make_prbs_intXOR).  seed in [0, 2^order), bit 0 = element 0 of the reference's bool seed; 0 <= start <= 2^62; 1 <= n <= 2^31; anything
 * else: QH_ERR_ARG before a launch.  The work of a call does not depend on start. */
int qh_prbs_bits_dev(int order, int kind, int64_t seed, int64_t start, int invert, int64_t n, uint8_t *bits);
/* labels[s] = the nb bits of symbol s, the first one the most significant (SignalQAMGrayCoded._modulate), s in [0, nsym); a non-zero byte
 * is a one.  nb in [2, 10], 1 <= nsym <= 2^31.  Rows of whole symbols are one call: nsym counts all of them. */
int qh_bits_to_labels_dev(const uint8_t *bits, int64_t nsym, int nb, int32_t *labels);
/* the inverse: the low nb bits of every label, most significant first. */
int qh_labels_to_bits_dev(const int32_t *labels, int64_t nsym, int nb, uint8_t *bits);
/* symbols[s] = alphabet[label of symbol s] (0 for a label outside [0, M)); labels: written too unless NULL. */
int qh_modulate_bits_c64_dev(const uint8_t *bits, int64_t nsym, int nb, const void *alphabet, int M, void *symbols, int32_t *labels);
int qh_modulate_bits_c128_dev(const uint8_t *bits, int64_t nsym, int nb, const void *alphabet, int M, void *symbols, int32_t *labels);
/* One launch: PRBS bits start .. start + nsym nb - 1 (arguments as qh_prbs_bits_dev, nsym nb <= 2^31) -> labels -> symbols of one row.
 * M must be 2^nb.  labels (nsym) and bits (nsym nb) are written only if not NULL. */
int qh_prbs_symbols_c64_dev(int order, int kind, int64_t seed, int64_t start, int64_t nsym, int nb, const void *alphabet, int M, void *symbols,
                            int32_t *labels, uint8_t *bits);
int qh_prbs_symbols_c128_dev(int order, int kind, int64_t seed, int64_t start, int64_t nsym, int nb, const void *alphabet, int M, void *symbols,
                             int32_t *labels, uint8_t *bits);

/* ---- pilot frames (csrc/pilot.hip; qampy/signals.py:1494-1545, :1753-1804, qampy/core/pilotbased_receiver.py:32-73, :258-327,
 * qampy/phaserec.py:194-218).  Device pointers, enqueued on the current stream, nothing read back.  A frame of F symbols: S pilots (the
 * sequence), then payload with one phase pilot every R symbols, the first of them at position S; R == 0: the sequence only.  NP = S + (F - S) / R
 * pilots (R == 0: S) and ND = F - NP payload symbols per frame.  QH_ERR_ARG before a launch for S < 0, S > F, R < 0, R == 1 and (F - S) % R != 0.
 * Assemble: frame (nmodes, nframes F) from pilots (nmodes, NP), scaled by pilot_scale (product in double, rounded once), and payload
 * (nmodes, ND), repeated in every frame, or - own_payload != 0 - (nmodes, nframes ND), ND symbols per frame.  idx_frame (nmodes, nframes F),
 * unless NULL: the payload's labels (same shape as payload) in the frame's layout, -1 at the pilots. */
int qh_pilot_frame_c64_dev(const void *pilots, const void *payload, const int32_t *labels, int nmodes, int64_t F, int64_t S, int64_t R, int64_t nframes,
                           int own_payload, double pilot_scale, void *frame, int32_t *idx_frame);
int qh_pilot_frame_c128_dev(const void *pilots, const void *payload, const int32_t *labels, int nmodes, int64_t F, int64_t S, int64_t R, int64_t nframes,
                            int own_payload, double pilot_scale, void *frame, int32_t *idx_frame);
/* Take apart: the frames frames[0 .. nfr - 1] (device table; every one whole inside L - a frame that is not is left out) of the frame-aligned
 * rows E (nmodes, L) into payload (nmodes, nfr ND) and / or pilots (nmodes, nfr NP), in the order of the table; either may be NULL. */
int qh_pilot_split_c64_dev(const void *E, int nmodes, int64_t L, int64_t F, int64_t S, int64_t R, const int32_t *frames, int64_t nfr, void *payload,
                           void *pilots);
int qh_pilot_split_c128_dev(const void *E, int nmodes, int64_t L, int64_t F, int64_t S, int64_t R, const int32_t *frames, int64_t nfr, void *payload,
                            void *pilots);
/* phase (nmodes, n) float64 = unwrap(angle(E[:, pos_j] conj(sent[:, j % nref]))), j in [0, n): pilot j sits at pos_j = where[j % npf] + (j / npf) F,
 * where (npf, device) strictly increasing inside [0, F); n is the number of j < npf nframes with pos_j < span <= min(L, nframes F) (the caller
 * counts them; a position outside the span counts as a zero sample).  Angles in double for both precisions, np.unwrap as an exact integer prefix
 * sum of wrap counts. */
int qh_pilot_phase_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n,
                           const void *sent, int64_t nref, double *phase);
int qh_pilot_phase_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n,
                            const void *sent, int64_t nref, double *phase);
/* knot_phase (nmodes, n - N + 1): the centred moving average over N phases, every output a direct sum in double; N odd, 3 <= N <= min(n, 1023).
 * knot_pos (n - N + 1) int64, unless NULL: the position of the pilot in the middle of every window (where == NULL: pilot j sits at j). */
int qh_pilot_knots_dev(const double *phase, int nmodes, int64_t n, int N, const int64_t *where, int64_t npf, int64_t F, double *knot_phase, int64_t *knot_pos);
/* The two above, then np.interp of the knots to every symbol of [0, span) (constant outside the knots) and its removal:
 * trace (nmodes, span) in the signal's real type, Eout (nmodes, span) = E[:, :span] exp(-1j trace). */
int qh_pilot_cpe_c64_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n,
                         const void *sent, int64_t nref, int N, void *Eout, void *trace);
int qh_pilot_cpe_c128_dev(const void *E, int nmodes, int64_t L, const int64_t *where, int64_t npf, int64_t nframes, int64_t F, int64_t span, int64_t n,
                          const void *sent, int64_t nref, int N, void *Eout, void *trace);
/* Least-squares line through the unwrapped phase of rec against ref, both (nmodes, n), n >= 2: fit (nmodes, 2) = [slope / (2 pi), intercept];
 * fo (nmodes): every mode's own slope / (2 pi), or - average != 0 - their mean in every entry (what qh_comp_freq_offset_*_dev takes). */
int qh_pilot_foe_c64_dev(const void *rec, const void *ref, int nmodes, int64_t n, int average, double *fit, double *fo);
int qh_pilot_foe_c128_dev(const void *rec, const void *ref, int nmodes, int64_t n, int average, double *fit, double *fo);
/* phase (nmodes): the mean of the unwrapped phase of rec against ref, both (nmodes, n). */
int qh_pilot_const_phase_c64_dev(const void *rec, const void *ref, int nmodes, int64_t n, double *phase);
int qh_pilot_const_phase_c128_dev(const void *rec, const void *ref, int nmodes, int64_t n, double *phase);
/* out[m] = E[m] exp(-1j phi[m]), phi (nmodes) float64 in device memory; out may be E. */
int qh_rotate_rows_c64_dev(const void *E, int nmodes, int64_t L, const double *phi, void *out);
int qh_rotate_rows_c128_dev(const void *E, int nmodes, int64_t L, const double *phi, void *out);

/* ---- digital pre-compensation (csrc/precomp.hip; qampy/core/digital_pre_compensation.py, qampy/core/pythran_dsp.py:201-240).  Device pointers,
 * enqueued on the current stream, nothing read back, a repeated call bit-identical.  Rows are (nmodes, L).
 * Pattern index: lev[k] = argmin |x[k] - levels| (the first minimum wins a tie, a NaN sample gets level 0) and
 * p[i] = sum_j lev[(i - mem_len / 2 + j) mod L] M^(mem_len - 1 - j), j = 0 .. mem_len - 1, for any L >= 1.  Either two rail tables in device memory -
 * lev_I (MI float64, strictly increasing) decides the real parts into idx_I with M = MI, lev_Q (MQ, 2 <= MQ <= MI) the imaginary parts into idx_Q with
 * M = MQ, alphabet NULL - or one alphabet (M points as float64 re / im pairs, lev_I and lev_Q NULL; squared distances in double), and idx_I and idx_Q
 * get the same numbers.  Either index row may be NULL.  1 <= mem_len <= 15, 2 <= M <= 4096, M^mem_len <= 2^24 (MI^mem_len for rails). */
int qh_pattern_index_c64_dev(const void *E, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M,
                             int mem_len, int32_t *idx_I, int32_t *idx_Q);
int qh_pattern_index_c128_dev(const void *E, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M,
                              int mem_len, int32_t *idx_I, int32_t *idx_Q);
/* Average error per pattern: err = tx - rx (in double) at the positions where mask is not 0 (mask NULL: everywhere; mask_rows 1: one (L) mask for all
 * rows, mask_rows nmodes: (nmodes, L)); ea (nmodes, N) complex128 = sum_I[p] / max(nI[p], 1) + 1j sum_Q[p] / max(nQ[p], 1), nI and nQ (nmodes, N)
 * int32 the counts, so that tables of several captures can be merged.  An index outside [0, N) is left out.  The sums are 64-bit integers in fixed
 * point at a power-of-two scale chosen from the row's max |err|: at least 37 bits below that maximum per sample, the same bits on every call.
 * 1 <= L <= 2^24, 1 <= N <= 2^24; errors must be finite. */
int qh_lut_accumulate_c64_dev(const void *tx, const void *rx, int nmodes, int64_t L, const int32_t *idx_I, const int32_t *idx_Q, const uint8_t *mask,
                              int mask_rows, int64_t N, void *ea, int32_t *nI, int32_t *nQ);
int qh_lut_accumulate_c128_dev(const void *tx, const void *rx, int nmodes, int64_t L, const int32_t *idx_I, const int32_t *idx_Q, const uint8_t *mask,
                               int mask_rows, int64_t N, void *ea, int32_t *nI, int32_t *nQ);
/* out = sig + gain (ea[idx_I].re + 1j ea[idx_Q].im), formed in double and rounded once; out may be sig. */
int qh_lut_apply_c64_dev(const void *sig, int nmodes, int64_t L, const void *ea, int64_t N, const int32_t *idx_I, const int32_t *idx_Q, double gain, void *out);
int qh_lut_apply_c128_dev(const void *sig, int nmodes, int64_t L, const void *ea, int64_t N, const int32_t *idx_I, const int32_t *idx_Q, double gain, void *out);
/* The same with the indices of qh_pattern_index_*_dev formed on the fly from sig (no index row is written); N must be M^mem_len, and out another
 * buffer than sig (a window reads its neighbours). */
int qh_lut_predistort_c64_dev(const void *sig, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M,
                              int mem_len, const void *ea, int64_t N, double gain, void *out);
int qh_lut_predistort_c128_dev(const void *sig, int nmodes, int64_t L, const double *lev_I, int MI, const double *lev_Q, int MQ, const double *alphabet, int M,
                               int mem_len, const void *ea, int64_t N, double gain, void *out);
/* out = 2 vpi_re asin(re) + 1j 2 vpi_im asin(im), in double, rounded once; NaN where a part lies outside [-1, 1], and - as numpy's complex product
 * 1j im leaves it - also in the real part where the imaginary part is NaN.  clip > 0: both parts are clamped to
 * +-clip first (a NaN stays one); clip == 0: no clamp.  out may be sig. */
int qh_comp_mod_sin_c64_dev(const void *sig, int nmodes, int64_t L, double vpi_re, double vpi_im, double clip, void *out);
int qh_comp_mod_sin_c128_dev(const void *sig, int nmodes, int64_t L, double vpi_re, double vpi_im, double clip, void *out);
/* p_f (sim_len bins in fftfreq order, the field's dtype) of comp_dac_resp, built in double: n_f the raised-cosine power response of roll-off beta at
 * the symbol rate fb on the grid fftfreq(sim_len) fs, d_f the response of the nsec (1 .. 4) second-order sections sos (HOST pointer, nsec x 6, a0 = 1)
 * at 2 pi k / sim_len, alpha = noise sum(|d_f|^2 n_f fs / sim_len) summed in a fixed order, p_f = n_f conj(d_f) / (n_f |d_f|^2 + alpha).
 * 1 <= sim_len <= 2^24. */
int qh_dac_preemphasis_table_c64_dev(int64_t sim_len, double fb, double fs, double beta, double noise, const double *sos, int nsec, void *p_f);
int qh_dac_preemphasis_table_c128_dev(int64_t sim_len, double fb, double fs, double beta, double noise, const double *sos, int nsec, void *p_f);

/* ---- theory curves (csrc/metrics.hip, csrc/source.hip; qampy/theory.py cal_gmi / sim_mi_mc / generate_ps_symbols, qampy/core/pythran_dsp.py:181-197).
 * Device pointers unless said otherwise, enqueued on the current stream, nothing read back, a repeated call bit-identical.
 * Monte-Carlo noise: z (nsnr, ns), z[p][l] = (g0 + 1j g1) sqrt(1 / (2 snr[p])), snr (nsnr) float64 linear, (g0, g1) the two standard normals of Philox
 * counter (l low, l high, p, stream 3) under the key seed - every SNR point its own draws.  1 <= nsnr <= 65535, 1 <= ns <= 2^31. */
int qh_awgn_mc_noise_c64_dev(void *z, const double *snr, int nsnr, int64_t ns, uint64_t seed);
int qh_awgn_mc_noise_c128_dev(void *z, const double *snr, int nsnr, int64_t ns, uint64_t seed);
/* Monte-Carlo GMI and MI of the alphabet (M = 2^nbits points, nbits 1 .. 10, point g carries label g) at every SNR point over the draws z (nsnr, ns):
 * out (nsnr, 2 + nbits) float64 = [gmi, mi, gmi of bit 0 .. nbits - 1 (MSB first)], gmi = cal_gmi_mc's value for the draws z[p], mi = cal_mi_mc(z[p],
 * alphabet, 1 / snr[p]).  Every sum of exponentials is shifted by its own largest exponent: finite for any z and snr > 0.  The SNR points run in
 * batches that keep the workgroup partials within 32 MiB of the calling thread's scratch, which the qh_metrics_*_dev calls use too: the scratch
 * belongs to the host thread, not to a stream, so after qh_use_stream() a call here and a metrics call of the same thread on another library
 * stream must be ordered by the caller (an event, or qh_stream_sync). */
int qh_awgn_mc_c64_dev(const void *alphabet, int M, const double *snr, int nsnr, const void *z, int64_t ns, double *out);
int qh_awgn_mc_c128_dev(const void *alphabet, int M, const double *snr, int nsnr, const void *z, int64_t ns, double *out);
/* Probabilistically shaped symbols: out (nmodes, N) = level[i] + 1j level[q], i and q the number of entries of cdf that are <= u, u = word 2^-32 of
 * the Philox words x (i) and y (q) of counter (n low, n high, mode, stream 4) under the key seed.  level and cdf: HOST tables of L <= 64 float64
 * entries, cdf non-decreasing with cdf[L - 1] == 1.  labels (nmodes, N) int32, or NULL, receives label_table[i L + q], label_table (L, L) int32 in
 * device memory.  1 <= nmodes <= 65535, 1 <= N <= 2^31 (one workgroup per 1024 samples of a mode, no stride: the limit of the
 * other sources of csrc/source.hip). */
int qh_ps_symbols_c64_dev(void *out, int nmodes, int64_t N, const double *level, const double *cdf, int L, uint64_t seed, int32_t *labels,
                          const int32_t *label_table);
int qh_ps_symbols_c128_dev(void *out, int nmodes, int64_t N, const double *level, const double *cdf, int L, uint64_t seed, int32_t *labels,
                           const int32_t *label_table);

/* ---- blind signal quality (csrc/blind.hip; qampy/core/signal_quality.py:122-271 norm_to_s0, cal_evm, cal_snr_qam, cal_s0, cal_snr_blind_qpsk).
 * Device pointers, E (nrows, L) dense rows, enqueued on the current stream, nothing read back, no atomics: a repeated call is bit-identical.
 * 1 <= nrows <= 65535, L >= 1.  The workgroup partials live in the calling thread's scratch (see qh_awgn_mc_*_dev on streams).
 * Moments: block = 0: mom (nrows, 4) float64 = mean |E|^2, mean |E|^4, mean re, mean im of every row; block > 0: mom (nrows, L / block, 4), the
 * same of every whole block of `block` samples (a shorter tail is left out); block > L is an argument error.  Terms and sums in double. */
int qh_blind_moments_c64_dev(const void *E, int nrows, int64_t L, int64_t block, double *mom);
int qh_blind_moments_c128_dev(const void *E, int nrows, int64_t L, int64_t block, double *mom);
/* stats (n, 6) float64 = (r2, r4, S1, S2, snr, s0) from mom (n, 4): k = r2^2 / r4, S1 = 1 - 2 k - sqrt((2 - gamma)(2 k^2 - k)), S2 = gamma k - 1,
 * snr = S1 / S2 (linear), s0 = r2 / (1 + S2 / S1); gamma = mean |a|^4 of the unit-power alphabet.  NaN / inf where the formula gives them. */
int qh_blind_finish_dev(const double *mom, int64_t n, double gamma, double *stats);
/* out = E / sqrt(stats[row][5]) in the precision of the row; out may be E. */
int qh_scale_by_stat_c64_dev(const void *E, int nrows, int64_t L, const double *stats, void *out);
int qh_scale_by_stat_c128_dev(const void *E, int nrows, int64_t L, const double *stats, void *out);
/* evm_sum (nrows) float64: known NULL: the sum over a row's samples of min_j |E / sqrt(stats[row][5]) - alphabet[j]|^2, alphabet M <= 1024 points
 * of E's type (already normalised); else the sum of |known / sqrt(stats_known[row][5]) - E / sqrt(stats[row][5])|^2, known (nrows, L) of E's type
 * (alphabet and M are then ignored).  Distances in the precision of the row, sums in double. */
int qh_blind_evm_c64_dev(const void *E, int nrows, int64_t L, const double *stats, const void *alphabet, int M, const void *known,
                         const double *stats_known, double *evm_sum);
int qh_blind_evm_c128_dev(const void *E, int nrows, int64_t L, const double *stats, const void *alphabet, int M, const void *known,
                          const double *stats_known, double *evm_sum);
/* out (nrows, 3) float64, or (nrows, L / block, 3) with block > 0 as above: P = mean |Eref|^2, var = P - |mean Eref|^2, 10 log10(P / var),
 * Eref = (-E^4)^(1/4) on the principal branch. */
int qh_qpsk_blind_c64_dev(const void *E, int nrows, int64_t L, int64_t block, double *out);
int qh_qpsk_blind_c128_dev(const void *E, int nrows, int64_t L, int64_t block, double *out);

/* ---- time-domain hybrid QAM (csrc/hybrid.hip; qampy/signals.py:1182-1427 TDHQAMSymbols, finished: DESIGN.md 3.21).  Two formats share a frame of
 * fM symbols, 2 <= fM <= 256: position n of a row carries format 1 when n % fM < fM1 (1 <= fM1 < fM), else format 2, whose symbols are stored
 * divided by sqrt(powratio) (powratio > 0, finite).  Device pointers, rows of whole frames (L % fM == 0, fM <= L < 2^31), 1 <= nmodes <= 65535,
 * enqueued on the current stream, nothing read back, no atomics: a repeated call is bit-identical.  Partials live in the calling thread's scratch.
 * Assemble: out (nmodes, nframes fM) from part1 (nmodes, nframes fM1) and part2 (nmodes, nframes fM2), part2 times 1 / sqrt(powratio) (the product
 * in double, rounded once); lab1, lab2 (int32, the parts' shapes) and idx_out (nmodes, nframes fM) int32 all given or all NULL: the labels laid
 * out like the symbols.  out must not be one of the parts. */
int qh_tdh_assemble_c64_dev(const void *part1, const void *part2, const int32_t *lab1, const int32_t *lab2, int nmodes, int64_t nframes, int fM, int fM1,
                            double powratio, void *out, int32_t *idx_out);
int qh_tdh_assemble_c128_dev(const void *part1, const void *part2, const int32_t *lab1, const int32_t *lab2, int nmodes, int64_t nframes, int fM, int fM1,
                             double powratio, void *out, int32_t *idx_out);
/* sums (nmodes, fM) float64: the sum of |E[row][n]| over n = r (mod fM), terms and sums in double, in a fixed order. */
int qh_tdh_class_sums_c64_dev(const void *E, int nmodes, int64_t L, int fM, double *sums);
int qh_tdh_class_sums_c128_dev(const void *E, int nmodes, int64_t L, int fM, double *sums);
/* shift (nmodes) int32 from the class sums: with H the residues of the higher-order format - [0, fM1) when high_first, else [fM1, fM) - the first j
 * in [0, fM) at which the sum over r in H of sums[row][(r + j) % fM] is strictly largest. */
int qh_tdh_align_dev(const double *sums, int nmodes, int fM, int fM1, int high_first, int32_t *shift);
/* part1[k] = E[(idx1[k] + shift) % L], part2[k] = E[(idx2[k] + shift) % L] sqrt(powratio), idx1 / idx2 the positions of the two formats in a row;
 * shift: shift_dev[row] (int32, device) when shift_dev is given, else shift_host for every row.  The parts must not be E. */
int qh_tdh_split_c64_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, void *part1,
                         void *part2);
int qh_tdh_split_c128_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host, void *part1,
                          void *part2);
/* sums (nmodes, 8) float64 = (symbol errors, bit errors, symbols compared, sum |r - s_label|^2) of format 1, then of format 2: r = E[(n + shift) % L],
 * times sqrt(powratio) in format 2, decided against the alphabet of position n (the nearest point by squared distance in E's precision, the first
 * on a tie) and compared with idx_tx[row][n], the label into that alphabet (nmodes, L) int32; bit errors are popc(decision ^ label).  A label
 * outside [0, M) is skipped.  alphabet1 (M1) and alphabet2 (M2) of E's type, 1 <= M <= 1024.  shift as in the split. */
int qh_tdh_metrics_c64_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host,
                           const int32_t *idx_tx, const void *alphabet1, int M1, const void *alphabet2, int M2, double *sums);
int qh_tdh_metrics_c128_dev(const void *E, int nmodes, int64_t L, int fM, int fM1, double powratio, const int32_t *shift_dev, int shift_host,
                            const int32_t *idx_tx, const void *alphabet1, int M1, const void *alphabet2, int M2, double *sums);

/* ---- nonlinear fibre (csrc/fibre.hip): symmetric split-step Fourier propagation of the (Manakov) nonlinear Schroedinger equation
 * over nspans identical amplified spans, and digital back-propagation.  E, out (nmodes, L) device pointers, out may be E; nmodes 1 (kappa = 1) or
 * 2 (kappa = 8 / 9); L a length qh_fft_*_dev takes.  dz: HOST table of the nsteps step lengths of one span in metres; f = fftfreq(L, 1 / fs);
 * beta2 in s^2 / m (add_dispersion's D wl0^2 / (2 pi c)), gamma in 1 / (W m), alpha in 1 / m.
 *   D(h)  every row becomes ifft(exp(-2 pi i t) . fft(row)), t = pi beta2 h f^2 turns, formed and reduced modulo one in double: exp(-0.5j w^2 beta2 h)
 *   N(h)  P[n] = sum_m |E[m, n]|^2, E[m, n] <- a exp(+j kappa gamma pscale h_eff P[n]) E[m, n], h_eff = (1 - exp(-alpha h)) / alpha (h for
 *         alpha == 0), a = exp(-alpha h / 2); the phase and the rotator are formed in the field's real type
 *   span  D(dz[0] / 2), then for i = 0 .. nsteps - 1: N(dz[i]), D(dz[i] / 2 + dz[i + 1] / 2), the last one D(dz[nsteps - 1] / 2): nsteps point-wise
 *         launches and nsteps + 1 filters (qh_spectral_filter_*_dev, kind 6); half steps are merged inside a span, never across spans
 * amplify != 0: the last N of a span also multiplies by exp(+alpha span / 2), span = sum dz: the lumped amplifier.  ase_w > 0 (watts per mode,
 * forward only): that launch then adds sigma w[m, n], sigma^2 = ase_w / pscale, w the unit noise of qh_impair_pointwise_*_dev (noise_mode 1,
 * sigma 1) under the seed `seed + s` (modulo 2^64) for span s.  pscale, watts per unit of |E|^2, is fixed once at the start and stays on the
 * device: power_mode 0: pscale = power; 1: pscale = power / sum_m mean_n |E[m, n]|^2, power the launch power over all rows in watts (two
 * launches, double, fixed order).  The field's normalisation is never changed.
 * backward != 0: the algebraic inverse of the noise-free forward call with the same arguments - steps reversed, beta2, gamma and alpha negated,
 * with amplify the factor exp(-alpha span / 2) in front of the first N of a span, before its power is taken.
 * QH_ERR_ARG before any launch: nmodes not 1 or 2, a length the transforms do not take, nsteps or nspans outside 1 .. 4096, a step that is not
 * finite and positive, a non-finite parameter, fs <= 0, ase_w < 0, ase_w != 0 with backward, power <= 0.  The whole loop is enqueued on the current
 * stream, nothing is read back, no atomics: a repeated call is bit-identical. */
int qh_fibre_ssfm_c64_dev(const void *E, int nmodes, int64_t L, double fs, double beta2, double gamma, double alpha, const double *dz, int nsteps,
                          int nspans, int backward, int amplify, int power_mode, double power, double ase_w, uint64_t seed, void *out);
int qh_fibre_ssfm_c128_dev(const void *E, int nmodes, int64_t L, double fs, double beta2, double gamma, double alpha, const double *dz, int nsteps,
                           int nspans, int backward, int amplify, int power_mode, double power, double ase_w, uint64_t seed, void *out);
/* The nonlinear step of the above on its own, one launch: out[m, n] = a exp(+j coef pscale[0] P[n]) E[m, n] (+ sigma w[m, n] when sigma_w > 0,
 * sigma = sigma_w / sqrt(pscale[0]), w as above under `seed`), P[n] = sum_m |E[m, n]|^2; pscale: one double in DEVICE memory.  nmodes 1 or 2,
 * 1 <= L <= 2^24; out may be E. */
int qh_fibre_nl_c64_dev(const void *E, int nmodes, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed, void *out);
int qh_fibre_nl_c128_dev(const void *E, int nmodes, int64_t L, double a, double coef, const double *pscale, double sigma_w, uint64_t seed, void *out);

#ifdef __cplusplus
}
#endif
#endif
