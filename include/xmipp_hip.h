/*
 * xmipp_hip.h -- C ABI of libxmipp_hip.so: the MI355X (gfx950) device side of
 * Xmipp's projection-matching + Fourier-gridding hot path.
 *
 * This is the drop-in boundary.  Host programs (our C++ mirrors of
 * ProgAngularProjectionMatching / ProgRecFourierAccel in xmipp3_amd/host, the
 * Python harness in xmipp3_amd/, or upstream Xmipp itself -- see
 * INTEGRATION.md) call only these entry points.  Plain pointers and sizes, no
 * C++/torch types.  Reference paths below are relative to
 * /root/reference/src/xmipp/libraries.
 *
 * Conventions
 *  - every function returns 0 on success, a negative xh_status otherwise;
 *    xh_last_error() gives the message (thread-local).  There is NO CPU
 *    fallback: without a usable HIP device xh_ctx_create fails.
 *  - pointers named d_* are device pointers (HBM) valid on the context's
 *    device, h_* are host pointers.  Device buffers may be owned by the caller
 *    (e.g. a torch tensor) -- the library never frees caller memory.
 *  - all work is enqueued on the context's HIP stream; calls return when the
 *    work is enqueued unless stated otherwise ("synchronous").
 *  - one host thread at a time per context; handles are not thread-safe (same
 *    contract as reconstruction_cuda/cuda_gpu_reconstruct_fourier.h:46-157, one
 *    stream per host thread).  Every entry point makes its context's device
 *    current on the calling thread, so a process may drive several devices
 *    from several threads (xmipp3_amd/host: --gpus).
 *  - images are row-major float32, D x D, logical (Xmipp) origin at pixel
 *    (D/2, D/2) as after MultidimArray::setXmippOrigin().
 */
#ifndef XMIPP_HIP_H
#define XMIPP_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    XH_OK = 0,
    XH_ERR_ARG = -1,     /* invalid argument / unsupported size */
    XH_ERR_HIP = -2,     /* HIP runtime error */
    XH_ERR_NOMEM = -3,
    XH_ERR_STATE = -4,   /* call made in the wrong state */
    XH_ERR_UNSUPPORTED = -5
} xh_status;

const char *xh_last_error(void);
const char *xh_version(void);

/* ------------------------------------------------------------------ context
 * Replaces createStreams/deleteStreams/waitForGPU
 * (reconstruction_cuda/cuda_gpu_reconstruct_fourier.h:46-60, :128) and the
 * GPU HW object (reconstruction_cuda/gpu.h:36-). */
typedef struct xh_ctx xh_ctx;
/* stream: the hipStream_t all work of this context is enqueued on (e.g. torch's current
 * stream); NULL means the device's default (null) stream. The stream stays owned by the caller. */
int xh_ctx_create(int device, void *stream, xh_ctx **out);
/* same, but the context creates (and destroys) a private non-blocking stream */
int xh_ctx_create_private(int device, xh_ctx **out);
int xh_ctx_destroy(xh_ctx *ctx);
int xh_ctx_sync(xh_ctx *ctx);                 /* synchronous: waits for the stream */
void *xh_ctx_stream(xh_ctx *ctx);
int xh_device_count(int *count);
/* NUMA node of the host the device hangs off (/sys/bus/pci/devices/<bus id>/numa_node), -1 when the platform does not say.
 * A host that feeds the device from threads on the other socket loses more than half of the H2D rate (measured: 21 instead of
 * 56 GB/s with 16 reader threads filling page-locked memory beside the copy), so the programs bind their loaders to it. */
int xh_device_numa_node(int device, int *node);
/* device memory helpers for hosts that do not bring their own allocator
 * (allocateTempVolumeGPU/releaseTempVolumeGPU, cuda_gpu_reconstruct_fourier.h:83-91) */
int xh_malloc(xh_ctx *ctx, size_t bytes, void **d_ptr);
int xh_free(xh_ctx *ctx, void *d_ptr);
int xh_memset(xh_ctx *ctx, void *d_ptr, int value, size_t bytes);
int xh_memcpy_h2d(xh_ctx *ctx, void *d_dst, const void *h_src, size_t bytes); /* synchronous */
int xh_memcpy_d2h(xh_ctx *ctx, void *h_dst, const void *d_src, size_t bytes); /* synchronous */
/* bytes of device memory the library's handles and calls hold right now, over all contexts of the process
 * (xh_malloc'd memory not included): every handle's destroy returns what it held */
int xh_device_bytes_held(int64_t *bytes);
/* Page-locked host memory and copies that only enqueue: what a loader thread needs to feed the device while it computes
 * (pinMemory / unpinMemory, cuda_gpu_reconstruct_fourier.h:134-136, gpu.h:78-113; the loader of
 * reconstruct_fourier_accel.cpp:300-388).  The async copies return when enqueued on the context's stream; the host
 * buffer must stay untouched until xh_ctx_sync (or a later synchronous call) on that context.  With pageable host
 * memory they are still correct, only not asynchronous. */
int xh_host_alloc(xh_ctx *ctx, size_t bytes, void **h_ptr);
int xh_host_free(xh_ctx *ctx, void *h_ptr);
int xh_memcpy_h2d_async(xh_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int xh_memcpy_d2h_async(xh_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* everything enqueued so far on `other`'s stream happens before what is enqueued on ctx's stream from now on
 * (an event recorded on one stream and waited for on the other; no host wait).  Both contexts on one device. */
int xh_ctx_wait_for(xh_ctx *ctx, xh_ctx *other);
/* elapsed-time probes on the context stream (HIP events), for bench.py's roofline object */
int xh_timer_create(xh_ctx *ctx, void **timer);
int xh_timer_start(xh_ctx *ctx, void *timer);
int xh_timer_stop(xh_ctx *ctx, void *timer);
int xh_timer_elapsed_ms(xh_ctx *ctx, void *timer, float *ms); /* synchronous */
int xh_timer_destroy(xh_ctx *ctx, void *timer);

/* ------------------------------------------------------- Fourier gridding
 * Replaces ProgRecFourierAccel's inner loops (reconstruction/
 * reconstruct_fourier_accel.cpp: preloadBuffer :300-388, cropAndShift :271-298,
 * preloadCTF :548-592, processProjection :710-763, processVoxelBlob :627-700,
 * processVoxel :595-625, mirrorAndCrop :853-887, finishComputations :1002-1055)
 * and the CUDA seam processBufferGPU/copyTempVolumes/copyBlobTable/copyConstants
 * (reconstruction_cuda/cuda_gpu_reconstruct_fourier.h:93-157). */
typedef struct {
    int32_t imgSize;            /* D; only square images (RFA:192-193) */
    double padding_proj;        /* --padding <proj> (RFA:65,91) */
    double padding_vol;         /* --padding <vol> */
    double max_resolution;      /* --max_resolution, digital frequency (RFA:66) */
    double blob_radius;         /* --blob radius order alpha (RFA:68) */
    int32_t blob_order;
    double blob_alpha;
    int32_t use_fast;           /* --fast */
    int32_t phase_flipped;      /* --phaseFlipped */
    double min_ctf;             /* --minCTF */
    double sampling;            /* --sampling Ts (A/px); iTs = 1/Ts */
} xh_rf_params;

/* CTFDescription fields used by getValuePureNoKAt (data/ctf.h:452-502,
 * data/ctf.cpp:645-679,1392-1402); defaults via xh_ctf_defaults
 * (data/ctf.cpp:365-388). */
typedef struct {
    double Tm, kV, DeltafU, DeltafV, azimuthal_angle, Cs, Ca, espr, ispr, alpha, DeltaF, DeltaR,
        Q0, K, envR0, envR1, envR2, phase_shift, VPP_radius;
} xh_ctf_params;
void xh_ctf_defaults(xh_ctf_params *p);

/* One projection x symmetry placement ("traverse space",
 * reconstruction/reconstruct_fourier_projection_traverse_space.h:37-59). The
 * library fills these itself from Euler angles; exposed for hosts that
 * already hold matrices. */
typedef struct xh_rf xh_rf;

int xh_rf_create(xh_ctx *ctx, const xh_rf_params *p, xh_rf **out);
int xh_rf_destroy(xh_rf *rf);
/* profiling / A-B knobs of the reconstruction handle (defaults are the product path): "ctf_fast" 1 | 0 (CTFs without envelope terms evaluated
 * by the cheap form of preloadCTF's value, or the general double-precision formula for every pixel), "order_spaces" 1 | 0 (the traverse
 * spaces of a launch ordered by plane -- the gridding kernel then shares the voxel queue between projections of one direction -- or in
 * input order; the order permutes the launch's float additions), "shift_bands" 1 | 0 (256-px images shifted band by band out of LDS, or
 * by k_rf_shift: same bits), "tile_max_spaces". Unknown names fail with XH_ERR_ARG. */
int xh_rf_set_option(xh_rf *rf, const char *name, double value);
/* derived sizes (RFA:196-199): paddedImgSize P, maxVolumeIndexYZ mv, fft crop sizeX=mv/2, sizeY=mv */
int xh_rf_sizes(const xh_rf *rf, int32_t *paddedImgSize, int32_t *maxVolumeIndex,
                int32_t *fftSizeX, int32_t *fftSizeY);
/* host copies of the lookup tables (RFA:201-239): blobTableSqrt[10000] float,
 * Fourier_blob_table[10000] double, iDeltaSqrt, iDeltaFourier */
int xh_rf_tables(const xh_rf *rf, float *h_blobTableSqrt, double *h_fourierBlobTable,
                 float *iDeltaSqrt, float *iDeltaFourier);
/* Temp spaces: one contiguous float buffer [ volume (mv+1)^3 complex | weights (mv+1)^3 ],
 * i.e. 3*(mv+1)^3 floats, layout [z][y][x]. By default owned by the handle; a caller-owned
 * buffer (e.g. a torch tensor, so torch.distributed can all-reduce it) can be attached
 * instead. xh_rf_reset zeroes it. */
size_t xh_rf_temp_floats(const xh_rf *rf);
int xh_rf_attach_temp(xh_rf *rf, float *d_temp /* xh_rf_temp_floats() floats */);
int xh_rf_temp_ptr(xh_rf *rf, float **d_temp);
int xh_rf_reset(xh_rf *rf);
/* Image::readApplyGeo(..., only_apply_shifts) (RFA:304-323): out = in translated by
 * h_shiftXY[i] = (shiftX, shiftY) pixels (and mirrored in x where h_flip[i] != 0; h_flip may be
 * NULL), cubic B-spline interpolation with wrapping. */
int xh_rf_shift_images(xh_rf *rf, const float *d_imgs, const float *h_shiftXY /* [n][2] */,
                       const uint8_t *h_flip /* [n] or NULL */, int32_t n, float *d_out);
/* The same from cubic B-spline coefficients the caller already holds (produceSplineCoefficients of
 * d_imgs, [n][D][D] float): in one refinement iteration the matcher has just computed them for the same
 * particles (xh_pm_last_coefficients), the reference's two programs each compute their own
 * (APM:569, RFA:304-323 through readApplyGeo). */
int xh_rf_shift_images_coefs(xh_rf *rf, const float *d_imgs, const float *d_coefs, const float *h_shiftXY,
                             const uint8_t *h_flip, int32_t n, float *d_out);
/* The same with the shifts and flips where xh_pm_translate / xh_pm_match left them (device memory: d_shiftX, d_shiftY
 * [n] doubles, d_flip [n] bytes or NULL; d_coefs may be NULL): no host copy of the matcher's outputs is needed
 * between the two programs (the reference passes them through a metadata file, APM:820-880 -> RFA:296-323). */
int xh_rf_shift_images_dev(xh_rf *rf, const float *d_imgs, const float *d_coefs, const double *d_shiftX,
                           const double *d_shiftY, const uint8_t *d_flip, int32_t n, float *d_out);
/* preloadBuffer + cropAndShift for n images already shifted (shifts applied):
 * d_imgs [n][D][D] float  ->  d_fft [n][mv][mv/2] complex<float> (interleaved) */
int xh_rf_prepare_images(xh_rf *rf, const float *d_imgs, int32_t n, float *d_fft);
/* preloadCTF for n images: h_ctf [n] params -> d_ctf, d_mod [n][mv][mv/2] float */
int xh_rf_ctf_arrays(xh_rf *rf, const xh_ctf_params *h_ctf, int32_t n, float *d_ctf, float *d_mod);
/* processBuffer: insert n prepared projections. h_angles [n][3] = (rot,tilt,psi) degrees;
 * h_weights [n] or NULL (=1); h_sym [nsym][9] row-major symmetry matrices R (NULL => identity,
 * nsym=1; RFA:241-256); d_ctf/d_mod NULL => no CTF. */
int xh_rf_insert(xh_rf *rf, const float *d_fft, const float *d_ctf, const float *d_mod,
                 const double *h_angles, const float *h_weights, int32_t n, const double *h_sym,
                 int32_t nsym);
/* processBufferGPU in one call (the reference's device variant does the FFT on the device as well,
 * reconstruction_cuda/cuda_gpu_reconstruct_fourier.h:130-157, RFG:417-473): images with the shifts already
 * applied [n][D][D] float + CTF parameters (h_ctf [n], or NULL) + orientations (h_angles [n][3] rot, tilt, psi
 * in degrees) + weights (or NULL) + symmetry matrices -> temp spaces. Same result as xh_rf_ctf_arrays +
 * xh_rf_prepare_images + xh_rf_insert on scratch owned by the handle. */
int xh_rf_insert_images(xh_rf *rf, const float *d_imgs, const xh_ctf_params *h_ctf, const double *h_angles,
                        const float *h_weights, int32_t n, const double *h_sym, int32_t nsym);
/* xh_rf_insert_images with the orientations where the matcher left them: d_angles [n][3] doubles (rot, tilt, psi in
 * degrees) and d_weights [n] floats (or NULL) in device memory. The traverse spaces (RFA:939-966, 430-522) are built
 * by a kernel from the functions the host path uses (double arithmetic on both sides, the device's fused multiply-adds
 * may round the last bit of a matrix element differently), so the two forms give the same temp spaces to float rounding
 * (test_device_side_orientations_give_the_host_forms_temp_spaces: 1e-6); a weight of 0 drops the projection (RFA:327-329). The call enqueues and returns: it never waits for the stream. */
int xh_rf_insert_images_dev(xh_rf *rf, const float *d_imgs, const xh_ctf_params *h_ctf, const double *d_angles,
                            const float *d_weights, int32_t n, const double *h_sym, int32_t nsym);
/* same but taking the 3x3 "localAInv" (= Euler^T) matrices directly, h_ainv [n][9] */
int xh_rf_insert_matrices(xh_rf *rf, const float *d_fft, const float *d_ctf, const float *d_mod,
                          const double *h_ainv, const float *h_weights, int32_t n,
                          const double *h_sym, int32_t nsym);
/* HIP-event time (ms, on the context's stream) and number of launches of the output-stationary
 * gridding kernel since the last reset -- the live per-launch duration behind bench.py's roofline.
 * No reference counterpart (RFG times nothing). */
int xh_rf_kernel_ms(xh_rf *rf, double *h_ms, int64_t *h_launches, int32_t reset);
/* mirrorAndCropTempSpaces (RFA:853-887): temp -> cropped [ (mv+1)^2*(mv/2+1) complex | weights ]
 * stored at the start of the same buffer; 3*(mv+1)^2*(mv/2+1) floats are what a multi-GPU
 * host all-reduces (SUM) before xh_rf_finish. */
int xh_rf_mirror_and_crop(xh_rf *rf);
size_t xh_rf_cropped_floats(const xh_rf *rf);
/* The cropped spaces as data (xh_rf_cropped_floats() floats on the handle's device):
 *  - export: copy them out (asynchronous on the handle's stream);
 *  - import: load (add = 0; the handle then counts as cropped) or accumulate (add != 0) a buffer of
 *    the same layout that lives on the handle's device.
 * This is what ProgRecFourier's --prepare_fsc does through its <fsc>_1_Fourier.vol / _1_Weights.vol
 * files (reconstruction/reconstruct_fourier.cpp:991-1045): keep half 1, rebuild from zero for half 2,
 * then sum both. xh_rf_finish consumes the cropped spaces (weights are divided in place), so export
 * before finishing whatever has to be summed later. */
int xh_rf_cropped_export(xh_rf *rf, float *d_dst);
int xh_rf_cropped_import(xh_rf *rf, const float *d_src, int32_t add);
/* Sum the cropped spaces of n handles (any mix of devices of this node) into rfs[0]; synchronous. Handles
 * that share a device are added there first; the first handle of every device then takes part in ONE
 * in-place RCCL all-reduce (ncclCommInitAll over the devices, grouped ncclAllReduce, float sum) over all
 * xGMI links, so each of those ends up with the total. RCCL is bound at run time; if it cannot be loaded
 * or initialised the call says so on stderr and falls back to a binary tree of peer copies + adds. Replaces
 * the 2*(mv+1)^2 MPI_Reduce calls of mpi_reconstruct_fourier_accel.cpp:245-266 (GPU variant:
 * parallel_adapt_cuda/mpi_reconstruct_fourier_gpu.cpp:250-268) for a single-process, thread-per-device
 * host (the torch.distributed host all-reduces the same buffer instead, see xh_rf_attach_temp). */
int xh_rf_reduce(xh_rf *const *rfs, int32_t n);
/* finishComputations (RFA:1002-1055): synchronous; writes D^3 doubles, [z][y][x] */
int xh_rf_finish(xh_rf *rf, double *h_volume);

/* ---------------------------------------------------- projection matching
 * Replaces ProgAngularProjectionMatching's inner loops (reconstruction/
 * angular_projection_matching.cpp: getCurrentReference :408-528,
 * threadRotationallyAlignOneImage :530-773, translationallyAlignOneImage :776-868)
 * and the primitives under them (data/polar.h:488-534,625-738, data/polar.cpp:34-148,
 * data/filters.cpp:1593-1752). */
typedef struct xh_pm xh_pm;
/* Builds the reference library on the device: d_refs [nrefs][D][D] float. Ri<1 -> 1,
 * Ro<0 -> D/2-1 (APM:266-274). h_Mctf: optional real filter [paddim][paddim] in FFT order
 * applied to every reference (APM:457-481), NULL for none. */
int xh_pm_create(xh_ctx *ctx, int32_t D, int32_t Ri, int32_t Ro, int32_t nrefs,
                 const float *d_refs, const double *h_Mctf, int32_t paddim, xh_pm **out);
int xh_pm_destroy(xh_pm *pm);
int xh_pm_info(const xh_pm *pm, int32_t *nsam_outer /*N*/, int32_t *ncoef, int32_t *nsamples);
/* Rotational search for n particles (d_particles [n][D][D] float), --thr 1 semantics.
 * Neighbour lists in CSR form on the HOST: h_nbr_off [n+1], h_nbr_ids; both NULL => every
 * particle is compared with references 0..nrefs-1 (dense mode).
 * first_image_parity: 0 if the first particle of this call is an even-numbered image of the
 * run (the visiting order of references flips per image, APM:615-626,1112).
 * Outputs (device, one per particle): refno (-1 if the list is empty), psi_idx in [0,N)
 * (psi = psi_idx*360/N, polar.cpp:145-147), flip.
 * The orientation indices are exact w.r.t. a double-precision evaluation: an fp32 coarse
 * pass ranks all (ref, angle, mirror) candidates and every particle whose runner-up lies
 * within the fp32 error margin of the winner is re-scored in fp64. */
int xh_pm_match(xh_pm *pm, const float *d_particles, int32_t n, const int32_t *h_nbr_off,
                const int32_t *h_nbr_ids, int32_t first_image_parity, int32_t *d_refno,
                int32_t *d_psi_idx, uint8_t *d_flip);
/* The general search of threadRotationallyAlignOneImage (APM:530-760), replacing its
 * `--search5d_shift/--search5d_step` and `--number_orientations` loops:
 *  ntrans > 0: 5-D search -- every particle is also resampled about (xoff5d[t], yoff5d[t])
 *    (the list built at APM:334-348) and every (reference, translation) pair is a row of the
 *    search; as in the reference only (refno, psi, flip) of the winner are kept (the shift is
 *    re-estimated by xh_pm_translate). ntrans == 0 is the single translation (0,0).
 *  n_orient > 1: the reference's running top-N (APM:714-735) evaluated exactly (all rows in
 *    fp64); outputs are [n][n_orient], rank-major per particle, refno = -1 for ranks that were
 *    never filled (counterValidCorrs, APM:1068-1090). n_orient <= 16.
 * xh_pm_match(...) == xh_pm_match_ex(..., 1, 0, NULL, NULL, ...). */
int xh_pm_match_ex(xh_pm *pm, const float *d_particles, int32_t n, const int32_t *h_nbr_off,
                   const int32_t *h_nbr_ids, int32_t first_image_parity, int32_t n_orient,
                   int32_t ntrans, const int32_t *h_xoff5d, const int32_t *h_yoff5d,
                   int32_t *d_refno, int32_t *d_psi_idx, uint8_t *d_flip);
/* Translational step for the winners (APM:776-868): bestShift on correlation_matrix(rotated
 * reference, (mirrored) particle), rejection beyond max_shift (<0 => D/2), translate+
 * correlationIndex => maxCC. fp64 on the device. Outputs device double [n]. */
int xh_pm_translate(xh_pm *pm, const float *d_particles, int32_t n, const int32_t *d_refno,
                    const int32_t *d_psi_idx, const uint8_t *d_flip, double max_shift,
                    double *d_shiftX, double *d_shiftY, double *d_maxCC);
/* fp32 cubic B-spline coefficients (produceSplineCoefficients, APM:569) of the particles of the last
 * xh_pm_match[_ex] call, [count][D][D] float on the device, valid until the next call on this handle;
 * first = index of the first particle they belong to (0 and count = n when the call ran in one chunk). */
int xh_pm_last_coefficients(const xh_pm *pm, const float **d_coefs, int32_t *first, int32_t *count);
/* particles the last xh_pm_translate repeated in double precision: its first pass is fp32 and a particle whose arg-max
 * or window decision (FIL:1659-1689) comes within a margin of flipping is done again in the reference's arithmetic
 * (xh_pm_set_option "s6_fp32" 0: everything in double; "s6_eps": the margin, relative to the map's maximum -- default 6.4e-6,
 * twenty times the measured error of the fp32 map). That error holds at any scale of particles and references: each image
 * enters the packed transforms scaled by the power of two that brings its RMS into [0.5, 1), exactly undone on its map, so
 * the supported range is an RMS within 2^-64 .. 2^64 of 1 for every particle and reference, in any ratio to each other
 * (tests/test_gpu_pm_scale.py holds 1e-3 .. 1e3 either way). A particle whose pixels are all equal (unmirrored, or zero)
 * or an all-zero reference gets the reference's shift for a constant map, (0, 0). Repeats are ordered: the same input gives
 * the same bits from run to run.
 * "s6_layout" 1 | 0: between its row and column transforms the fp32 pass keeps the spectra column-major (a column is one run in
 * memory, which the column pass reads and writes whole) or row-major (the earlier kernels, kept for comparison). Same arithmetic
 * in the same order: identical results either way. */
int xh_pm_translate_stats(const xh_pm *pm, int64_t *repeated);
/* statistics of the last xh_pm_match call: rows evaluated, particles re-scored in fp64 */
int xh_pm_last_stats(const xh_pm *pm, int64_t *rows, int64_t *rescored_particles,
                     int64_t *rescored_rows);
/* accumulated device time (HIP events) per stage of xh_pm_match since the last reset:
 * h_ms[8] = { prep32, contract, idft_max, select, rescore_fp64, 0, 0, 0 } milliseconds */
int xh_pm_stage_ms(xh_pm *pm, double *h_ms, int32_t reset);
/* rows of the last xh_pm_match[_ex] call that the S3 branch and bound skipped: a correlation row whose
 * coefficient moduli sum to less than (best value found for the particle - 2 tau) is never transformed.
 * Same results with set_option("prune", 0); no reference counterpart (the reference transforms every row,
 * polar.cpp:136-146). */
int xh_pm_rows_pruned(const xh_pm *pm, int64_t *rows_pruned);
/* Two-level contraction: the angular frequency K0 at which the MFMA contraction of the dense search stops
 * (the reference bank holds < 1e-5 of its summed coefficient norms above it); rows that survive the branch and
 * bound get their frequencies K0..nk-1 afterwards, a particle's rows together (set_option "group_high" 0: each by the wave
 * that transforms it), all others are covered by a Cauchy-Schwarz term in their bound. K0 == nk: the bank is not band
 * limited, everything is contracted. set_option("k0", v) overrides (0 = automatic). Identical results for every K0.
 * A gallery with flat correlation peaks leaves a large part of the rows standing: when more than 10 % of a chunk's rows
 * survive, the next chunk (of this or of the next call) is contracted at every frequency with its coefficients kept, which
 * is cheaper from 9 % on; below 6 % it goes back (set_option "adaptive_finish" 0: never; get_option "dense_chunks": how
 * many chunks of the last call took that form). Identical results either way.
 * Before the survivors' frequencies K0..nk-1 are contracted they are transformed from their frequencies below K0 alone: a row whose
 * low-only maximum plus its Cauchy-Schwarz term lies more than 2 tau below the best (low-only maximum - term) of the particle cannot
 * be the winner or a candidate of the re-score and is left out (set_option "low_pass" 0: every survivor is finished; identical
 * results either way). get_option "low_pass_rows_in" / "low_pass_rows_out": the survivors of the last call that this test looked at
 * and those it left to finish; "low_pass_rows_transformed": the low-only transforms it took (a particle's four planned rows had
 * theirs already). xh_pm_rows_pruned keeps counting the rows the sums of moduli skipped. */
int xh_pm_two_level_cut(const xh_pm *pm, int32_t *K0, int32_t *nk);
/* tuning knobs: "tau_rel" (fp32 ambiguity margin relative to sum_r 2*pi*r), "chunk_rows" (rows per launch chunk), "prune", "k0",
 * "mask_lists", "group_high", "low_pass", "high_cap", "adaptive_finish", "tr_chunk_mb", "s6_fp32", "s6_eps", "s6_layout", "s6_capture" (see above and below).
 * "threads" n (1..16): the reference program's --thr (angular_projection_matching.cpp:64,631,1018-1108).  Its n worker threads take
 * the positions i % n of a particle's neighbour list and their results are merged, worker 0 first, strictly greater wins -- which
 * only shows where two correlation values are EXACTLY equal (duplicated references): the winner is then the one with the smallest
 * (i % n, position in the image's visiting order) instead of the first visited.  xh_pm_match[_ex] reproduces that order, for the
 * running top-N (n_orient > 1) as well.  Unknown names fail with XH_ERR_ARG. */
int xh_pm_set_option(xh_pm *pm, const char *name, double value);
/* current value of "tau_rel" (ambiguity margin of the fp32 coarse search, relative to sum_r 2 pi r) or "s6_eps" (margin of the
 * fp32 pass of xh_pm_translate, relative to the maximum of the correlation map): the tests hold the measured fp32 errors against them;
 * "adaptive_finish", "dense_chunks", "low_pass", "low_pass_rows_in", "low_pass_rows_out", "low_pass_rows_transformed": see
 * xh_pm_two_level_cut; "s6_layout": see xh_pm_translate_stats */
int xh_pm_get_option(const xh_pm *pm, const char *name, double *value);

/* ---- FourierProjector: central-slice projections of a volume ------------------
 * Replaces the class FourierProjector (libraries/data/fourier_projection.h:111-172) behind
 * xmipp_angular_project_library --method fourier <pad> <maxfreq> bspline
 * (reconstruction/angular_project_library.cpp:194-245): the gallery of references that
 * xh_pm_create consumes, so that volume -> references -> match -> reconstruct stays on the device.
 *   create  == FourierProjector(V, paddFactor, maxFreq, BSPLINE3) / updateVolume
 *              (fourier_projection.cpp:72-89,247-330); d_vol: D^3 floats, [z][y][x], Xmipp origin.
 *   project == project(rot, tilt, psi, ctf) + projection() for n orientations at once
 *              (fourier_projection.cpp:91-245); h_angles: n x (rot, tilt, psi) degrees; d_ctf: optional
 *              [D][D/2+1] doubles multiplied onto the slice; d_out: n x D x D floats. n = 0 does nothing
 *              and reads neither pointer.
 * Only cubic B-spline interpolation (the program's default) is implemented; degree 0/1 fail loudly. */
typedef struct xh_fp xh_fp;
int xh_fp_create(xh_ctx *ctx, const float *d_vol, int32_t D, double padding, double max_freq,
                 int32_t degree, xh_fp **out);
int xh_fp_destroy(xh_fp *fp);
int xh_fp_info(const xh_fp *fp, int32_t *padded_size, int32_t *coef_dim, int32_t *coef_start);
/* test hook: the cropped B-spline coefficient cubes (VfourierRealCoefs / VfourierImagCoefs), host doubles */
int xh_fp_coefs(const xh_fp *fp, double *h_re, double *h_im);
int xh_fp_project(xh_fp *fp, const double *h_angles, int32_t n, const double *d_ctf, float *d_out);

/* ------------------------------------------------- Fourier shell correlation
 * Replaces the frc_dpr(refI(), img(), sam, freq, frc, frc_noise, dpr, error_l2, do_dpr, do_rfactor,
 * min_samp, sam/max_sam, &rFactor) call of ProgResolutionFsc::process_img
 * (reconstruction/resolution_fsc.cpp:179-203; frc_dpr itself is xmippCore's xmipp_fftw.cpp).
 * d_m1 (the reference map) and d_m2: [Z][Y][X] doubles on the device (Z = 1 for images), sizes <= 1024.
 * Outputs on the host, X/2+1 doubles each (h_dpr / h_rfactor only touched when requested): digital
 * frequency / sampling_rate, FRC, 2/sqrt(shell count), differential phase residual (degrees), mean
 * |F1 - F2|; R-factor over minFreq <= R <= maxFreq (digital frequencies). Synchronous. */
int xh_frc_dpr(xh_ctx *ctx, const double *d_m1, const double *d_m2, int32_t Z, int32_t Y, int32_t X,
               double sampling_rate, int32_t do_dpr, int32_t do_rfactor, double minFreq, double maxFreq,
               double *h_freq, double *h_frc, double *h_frc_noise, double *h_dpr, double *h_error_l2,
               double *h_rfactor);

/* ---- test hooks (used only by tests/ to localise a parity failure per stage) ---- */
/* polar Fourier transform of one stage: precision 32 or 64; outputs on host */
int xh_pm_debug_prepare(xh_pm *pm, const float *d_particles, int32_t n, int32_t precision,
                        double *h_coefs /* [n][ncoef][2] */, double *h_sigma /* [n] */);
int xh_pm_debug_ref(xh_pm *pm, int32_t ref, double *h_coefs /* [ncoef][2] conj'd */,
                    double *h_sigma);
/* full normalised correlation rows (straight || mirror, 2N) of particle p vs reference r as
 * computed by the fp32 coarse pass (precision 32) or the fp64 re-scorer (64) */
int xh_pm_debug_corr_rows(xh_pm *pm, const float *d_particle, int32_t ref, int32_t precision,
                          double *h_corr2N);
/* the correlation maps (correlation_matrix, FIL:1636) the last chunk of an xh_pm_translate call under
 * set_option("s6_capture", 32 | 64) left behind, [n][D][D] doubles on the host; 64, 128 and 256 px */
int xh_pm_debug_s6_maps(xh_pm *pm, int32_t n, double *h_maps);

/* ---- 2-D complex FFTs of whole movie frames (FlexAlign) --------------------------------
 * reconstruction_adapt_cuda/movie_alignment_correlation_gpu.cpp:633-725 plans cuFFT transforms of 4096 x 5760 (K3) frames;
 * a line of that length does not fit one LDS transform, so it is done in four steps (two strided passes of the line
 * kernels, a twiddle pass, an untangling transpose). ny x nx complex<float>, row-major, interleaved, in place;
 * forward un-normalised, inverse divided by ny nx (FFTW / cuFFT conventions of the reference's FourierTransformer:
 * forward/normalised-inverse pair). Any ny, nx whose prime factors allow a split into two lines of at most 2048 (powers
 * of two) / 1024 (other lengths, Bluestein) points: up to about a million points per axis. */
typedef struct xh_fft2d xh_fft2d;
int xh_fft2d_create(xh_ctx *ctx, int32_t ny, int32_t nx, xh_fft2d **out);
int xh_fft2d_destroy(xh_fft2d *f);
/* h_factors[4] = (ny1, ny2, nx1, nx2): the split of either axis (n2 = 1: one LDS transform per line) */
int xh_fft2d_factors(const xh_fft2d *f, int32_t *h_factors);
int xh_fft2d_exec(xh_fft2d *f, float *d_data /* [ny][nx][2] */, int32_t inverse);
int xh_fft2d_exec_axis(xh_fft2d *f, float *d_data, int32_t inverse, int32_t axis /* 0: rows only, 1: columns only; un-normalised */);

/* ---- test hooks (used only by tests/ to check the transforms every module builds on, path by path) ----
 * The LDS line transform of every separable FFT (xh_plan.h), un-normalised, in place on complex<float> (precision 32) or
 * complex<double> (64): nlines lines of n points, line l starting at (l / inner) * outerStride + (l % inner) * innerStride, its
 * elements elemStride apart (in complex elements); min(maxLines, 64 KB / line) lines per workgroup like the callers. A line whose
 * LDS form does not fit 64 KB is refused (XH_ERR_UNSUPPORTED). Synchronous. */
int xh_debug_fft_lines(xh_ctx *ctx, int32_t precision, int32_t n, void *d_data, size_t nlines, size_t inner, size_t outerStride,
                       size_t innerStride, size_t elemStride, int32_t maxLines, int32_t inverse);
/* FlexAlign's row pass of a real Y x X frame, (frame - dark) * gain, on a plan f = xh_fft2d_create(ctx, (Y + 1) / 2, X); dark / gain
 * nullable. form 0: the packed rows row[2r] + i row[2r + 1] transformed as [(Y + 1) / 2][X] complex, frequency k of a row at
 * n2 (k % n1) + k / n1; form 1: the nc lowest frequencies of every real row, [Y][nc] complex. h_info[3] = (n1, n2, done): done = 0
 * when the plan's rows do not take that form (nothing written). Synchronous. */
int xh_fft2d_debug_real_rows(xh_fft2d *f, const float *d_frame, const float *d_dark, const float *d_gain, int32_t Y, int32_t nc,
                             int32_t form, float *d_out, int32_t *h_info);

/* ---- ProgRecFourier's own arithmetic: the program behind xmipp_reconstruct_fourier ----------
 * reconstruction/reconstruct_fourier.cpp: double accumulators, image-driven scatter into the FFTW-layout Fourier volume with
 * wrap and, beyond the half, the point-mirrored conjugated slot (RF:571-793), correctWeight with its re-processing passes
 * (RF:1056-1101), enforceHermitianSymmetry + PROCESS_WEIGHTS + inverse transform + corrections (RF:451-480,1103-1178).
 *   create   == produceSideInfo (RF:184-287); niter_weight = --iter (0: weights set to one).
 *   insert   == processImages over n projections (shifts already applied, D x D floats on the device): their transform in
 *               double, then the scatter with double-precision atomics; h_ctf nullable (--useCTF, RF:600-625), h_angles
 *               (rot, tilt, psi), h_weights nullable, h_sym nsym x 9 nullable. reprocess != 0: the weight re-processing pass
 *               (images ignored).
 *   weights_step == correctWeight: 0 begin; per further iteration { 1; replay every projection with reprocess = 1; 2 }; 3 end.
 *   finish   == finishComputations -> D^3 doubles on the host; the Fourier volume and weights stay (state_export / import
 *               [F (2 nF) | W (nF)] doubles keep the halves of --prepare_fsc, RF:991-1045).
 * Built for exactness (BASELINE config 1's plumbing path); the accel program is the fast one. */
typedef struct xh_rf2 xh_rf2;
int xh_rf2_create(xh_ctx *ctx, const xh_rf_params *p, int32_t niter_weight, xh_rf2 **out);
int xh_rf2_destroy(xh_rf2 *h);
int xh_rf2_reset(xh_rf2 *h);
int xh_rf2_insert(xh_rf2 *h, const float *d_imgs, const xh_ctf_params *h_ctf, const double *h_angles, const float *h_weights, int32_t n,
                  const double *h_sym, int32_t nsym, int32_t reprocess);
int xh_rf2_weights_step(xh_rf2 *h, int32_t step);
size_t xh_rf2_state_doubles(const xh_rf2 *h);
int xh_rf2_state_export(xh_rf2 *h, double *d_dst);
int xh_rf2_state_import(xh_rf2 *h, const double *d_src, int32_t add);
int xh_rf2_finish(xh_rf2 *h, double *h_volume);

/* ---- CTF pre-steps -------------------------------------------------------------------
 * xmipp_ctf_phase_flip: actualPhaseFlip (reconstruction/ctf_phase_flip.cpp:88-117) -- the coefficients of a micrograph where
 * the undamped CTF (getValuePureWithoutDampingAt, data/ctf.h:541-570) is negative change sign.
 * xmipp_ctf_correct_wiener2d: Wiener2D::wienerFilter + applyWienerFilter (data/wiener2d.cpp:29-141) -- every particle is
 * padded about the Xmipp origin, multiplied in Fourier space by CTF / (CTF^2 + wc) (wc < 0: 0.1 mean CTF^2) and cropped back.
 * A handle serves images of one size: ydim x xdim floats on the device, in place; pad = 1 for phase flipping. CTF
 * descriptions on the host (phase_shift in degrees, as the metadata holds it); sampling_rate = Tm the CTF is evaluated at.
 * is_isotropic is accepted and, as in the reference (which averages the defoci after produceSideInfo has used them), has no
 * effect. CTF in double precision, transforms in fp32. */
typedef struct xh_ctfop xh_ctfop;
int xh_ctfop_create(xh_ctx *ctx, int32_t ydim, int32_t xdim, double pad, xh_ctfop **out);
int xh_ctfop_destroy(xh_ctfop *h);
int xh_ctfop_phase_flip(xh_ctfop *h, float *d_img, const xh_ctf_params *ctf, double sampling_rate);
int xh_ctfop_wiener2d(xh_ctfop *h, float *d_imgs /* [n][ydim][xdim] */, int32_t n, const xh_ctf_params *ctfs, double sampling_rate,
                      int32_t phase_flipped, int32_t is_isotropic, double wiener_constant, int32_t correct_envelope);

/* ---- FlexAlign: global alignment of a movie (BASELINE config 5, first slice) -----------
 * ProgMovieAlignmentCorrelationGPU<T>::computeGlobalAlignment (reconstruction_adapt_cuda/movie_alignment_correlation_gpu.cpp:
 * 633-725) with the arithmetic of the CPU program (reconstruction/movie_alignment_correlation.cpp:45-157, _base.cpp:152-320,
 * 399-418, eq_system_solver.cpp:35-106): dark / gain correction, Fourier-space reduction of every frame to the size the
 * maximal resolution needs, Gaussian low-pass, correlation of all frame pairs, bestShift within max_shift, least squares over
 * the pair shifts with outlier rejection, reference frame, shift of every frame from it.
 *   create: frames of Y x X pixels at sampling_rate A/px, --maxResForCorrelation A; fails when the scale factor is >= 1.
 *   global_alignment: d_frames [N][Y][X] float on the device, d_dark / d_gain [Y][X] or null, max_shift_px = --maxShift /
 *   sampling rate. Host outputs: pair shifts h_bX / h_bY [N (N-1)/2] (nullable; movie pixels, order (0,1), (0,2) ...),
 *   h_shiftX / h_shiftY [N] from the reference frame h_ref (what storeGlobalShifts negates into the metadata).
 *
 * Local (patch) alignment, ProgMovieAlignmentCorrelationGPU<T>::computeLocalAlignment (movie_alignment_correlation_gpu.cpp:
 * 288-430; the reference has it for CUDA only) and the output of the aligned movie (applyShiftsComputeAverage, :479-570):
 *   local_alignment: patches_x x patches_y patches of patch_size pixels (made even) laid out by getPatchesLocation over what
 *   the global shifts h_gShiftX/Y [N] leave of the frame; per patch the sum of patches_avg frames at their rounded global
 *   shift, reduced in Fourier space to the correlation size (getCorrelationHint: the smallest even size keeping the scale
 *   factor; the reference may pick a larger one after benchmarking cuFFT on the installed GPU), low-passed, all frame pairs
 *   correlated, first maximum within max_shift of the centre, 3 x 3 centre of mass, least squares per patch from frame
 *   ref_frame. Host outputs: h_patchShifts [patches_y][patches_x][N][2] (x, y; rounded global + local), h_centers
 *   [patches_y][patches_x][2], the B-spline coefficients h_coeffsX/Y [lT][lY][lX] of BSplineHelper::computeBSplineCoeffs
 *   (nullable), h_dims[4] = patch size x, y, correlation size x, y (nullable).
 *   local_from_global: localFromGlobal (:432-456), the B-spline of a movie aligned globally only.
 *   apply_bspline: frame n of N (d_frame [Y][X], dark / gain applied on the way) warped by the B-spline like
 *   GeoTransformer::applyBSplineTransform(3, ...) (cuda_gpu_geo_transformer.cpp:186-239): d_out = the aligned frame (nullable),
 *   d_sum += it (nullable), d_initial_sum += the corrected, unaligned frame (nullable). */
typedef struct xh_fa xh_fa;
int xh_fa_create(xh_ctx *ctx, int32_t Y, int32_t X, float sampling_rate, float max_res_for_correlation, xh_fa **out);
int xh_fa_destroy(xh_fa *h);
int xh_fa_info(const xh_fa *h, int32_t *newY, int32_t *newX, double *size_factor);
int xh_fa_set_option(xh_fa *h, const char *name, double value); /* "window" 0: every pair correlation through the full inverse transform (A/B);
                                                                  "pruned_columns" 0: the column pass of the frame transform as full-length line transforms (A/B; default 1:
                                                                  two steps that compute the rows the reduced frame keeps only, as small DFTs on the vector ALUs when Y
                                                                  has a divisor that allows it, else -- or with 2 -- as products on the matrix cores);
                                                                  "rows_kept" 0: the row pass of frames with 5760-point rows by the general kernels (A/B; default 1: one kernel that
                                                                  writes the kept columns only);
                                                                  "pairwin_form" 0: pair / patch correlation windows by the plain kernels (A/B; default 1: packed multiply-adds);
                                                                  "prefilter_ahead" 1: xh_fa_local_alignment ends with the warp's B-spline prefilter of every frame
                                                                  (N Y X floats kept with the handle), run while the host fits the spline; the following
                                                                  xh_fa_apply_bspline[_frames] calls on the same frames (without an initial sum) use it.
                                                                  CONTRACT: the frames are recognised by their device address (d_frames, d_dark, d_gain, N): a caller
                                                                  that rewrites d_frames in place after xh_fa_local_alignment must call it (or xh_fa_global_alignment)
                                                                  again, or switch the option off, before warping. When the device cannot spare the N Y X floats
                                                                  the option silently does nothing (the warp prefilters frame by frame).
                                                                  Control grids: a layer of lX x lY control points must fit 64 KB of LDS (lX lY <= 2048), else
                                                                  xh_fa_apply_bspline fails with XH_ERR_UNSUPPORTED */
int xh_fa_last_full_pairs(const xh_fa *h);                        /* pairs of the last global alignment that needed the full transform */
int xh_fa_global_alignment(xh_fa *h, const float *d_frames, int32_t N, const float *d_dark, const float *d_gain, float max_shift_px,
                           double *h_bX, double *h_bY, double *h_shiftX, double *h_shiftY, int32_t *h_ref);
int xh_fa_local_alignment(xh_fa *h, const float *d_frames, int32_t N, const float *d_dark, const float *d_gain, const double *h_gShiftX,
                          const double *h_gShiftY, int32_t ref_frame, float max_shift_px, int32_t patches_x, int32_t patches_y,
                          int32_t patch_size_x, int32_t patch_size_y, int32_t patches_avg, int32_t lX, int32_t lY, int32_t lT,
                          double *h_patchShifts, double *h_centers, double *h_coeffsX, double *h_coeffsY, int32_t *h_dims);
/* CUDAFlexAlignCorrelate<T>::run (reconstruction_cuda/cuda_flexalign_correlate.cpp:95-140): d_frames [N][Y][X] (even sizes) -> h_pos
 * [N (N-1)/2][2] = (x, y) of the correlation maximum of every pair i < j within max_dist of the centre (X/2, Y/2), refined over 3 x 3 */
int xh_fa_correlate(xh_ctx *ctx, const float *d_frames, int32_t N, int32_t Y, int32_t X, float max_dist, double *h_pos);
int xh_fa_local_from_global(xh_fa *h, int32_t N, const double *h_gShiftX, const double *h_gShiftY, int32_t patches_x, int32_t patches_y,
                            int32_t patch_size_x, int32_t patch_size_y, int32_t lX, int32_t lY, int32_t lT, double *h_centers,
                            double *h_coeffsX, double *h_coeffsY);
int xh_fa_apply_bspline(xh_fa *h, const float *d_frame, const float *d_dark, const float *d_gain, const double *h_coeffsX,
                        const double *h_coeffsY, int32_t lX, int32_t lY, int32_t lT, int32_t N, int32_t n, float *d_out, float *d_sum,
                        float *d_initial_sum);
/* the loop of applyShiftsComputeAverage (:479-560) in one call: frames n0 .. n1 of d_frames [N][Y][X] warped with their frame index and added
 * into d_sum / d_initial_sum (nullable); d_out_stack (nullable, [n1 - n0 + 1][Y][X]) receives the aligned frames */
int xh_fa_apply_bspline_frames(xh_fa *h, const float *d_frames, int32_t N, int32_t n0, int32_t n1, const float *d_dark, const float *d_gain,
                               const double *h_coeffsX, const double *h_coeffsY, int32_t lX, int32_t lY, int32_t lT, float *d_out_stack, float *d_sum,
                               float *d_initial_sum);

/* ProgMovieFilterDose::applyDoseFilterToImage between the two transforms of a frame (reconstruction/movie_filter_dose.cpp:85-170,
 * 283-287): d_frame [Y][X] in place; plan = xh_fft2d_create(ctx, Y, X); acc_voltage 200 or 300 kV (anything else is refused like
 * initVoltage does); dose_start / dose_finish = n / (n + 1) x dosePerFrame + preExposure of frame n. */
int xh_movie_dose_filter(xh_ctx *ctx, xh_fft2d *plan, float *d_frame, int32_t Y, int32_t X, double pixel_size, double acc_voltage,
                         double dose_start, double dose_finish);
/* --bin of the CUDA FlexAlign program: a frame binned while it is loaded (CUDAFlexAlignScale::runScaleIFT,
 * reconstruction_cuda/cuda_flexalign_scale.cpp:101-121; scaleFFT2DKernel, cuda_scaleFFT_kernels.cu:44-79; sizes from
 * AProgMovieAlignmentCorrelation::getMovieSize, reconstruction/movie_alignment_correlation_base.cpp:356-370): half spectrum of the
 * raw frame (minus d_dark, times d_gain: loadFrame corrects before it bins; either may be null) cropped to the binned size, times
 * 1 / (X Y), inverse transform.  d_frame [Y][X] -> d_out [Yb][Xb]; planRaw =
 * xh_fft2d_create(ctx, Y, X), planBinned = xh_fft2d_create(ctx, Yb, Xb). */
int xh_movie_bin_frame(xh_ctx *ctx, xh_fft2d *planRaw, xh_fft2d *planBinned, const float *d_frame, const float *d_dark, const float *d_gain, int32_t Y,
                       int32_t X, float *d_out, int32_t Yb, int32_t Xb);

/* The top-left cropY x cropX window of N frames of Y x X floats, frame after frame (getCroppedFrame,
 * reconstruction_adapt_cuda/movie_alignment_correlation_gpu.cpp:727-734: the CUDA program correlates frames cropped to an
 * FFT-friendly size, findGoodCropSize :73-88).  d_dst: N x cropY x cropX floats. */
int xh_movie_crop_frames(xh_ctx *ctx, const float *d_src, int32_t N, int32_t Y, int32_t X, int32_t cropY, int32_t cropX, float *d_dst);
/* A frame as the detector stores it -> float32 on the device: the cast Image<float>::read does on the host while it reads
 * (xmippCore rwMRC / castPage2T; the movie programs read through it, reconstruction/movie_alignment_correlation_base.cpp:262-266,
 * movie_alignment_correlation_gpu.cpp:667-691), moved behind the host copy so that counts cross the link, not floats.  mode: the MRC
 * data mode of the file -- 0 int8, 1 int16, 2 float32 (a copy), 6 uint16 -- or 100 for uint8 (not an MRC mode); n elements. */
int xh_movie_frame_to_float(xh_ctx *ctx, const void *d_raw, int32_t mode, int64_t n, float *d_out);

/* ---- batched estimator API, first slice ------------------------------------------------------
 * ExtremaFinder::SingleExtremaFinder<T> (reconstruction/single_extrema_finder.cpp:146-300): n signals [n][z][y][x] on the device;
 * search_type 0 Max, 1 Lowest (first of equals, like std::max_element / min_element), 2 MaxAroundCenter, 3 LowestAroundCenter (2-D
 * only: within max_dist of (x/2, y/2), first in raster order); h_positions [n] element offsets as floats (-1: nothing searched),
 * h_values [n]; either may be NULL. */
int xh_extrema_find(xh_ctx *ctx, const float *d_data, int32_t n, int32_t zdim, int32_t ydim, int32_t xdim, int32_t search_type, float max_dist,
                    float *h_positions, float *h_values);
/* Alignment::ShiftCorrEstimator<T>, AlignType::OneToN (reconstruction/shift_corr_estimator.cpp:33-300): create = init2D (even sizes,
 * 0 < max_shift < size / 2); load_reference = load2DReferenceOneToN(const T *); correlate = the static
 * computeCorrelations2DOneToN (d_inout [n][fy][fx] complex spectra <- ref conj(inout), times (-1)^(x+y) when center);
 * compute_shifts = computeShift2DOneToN + getShifts2D: h_shifts [n][2] = (x, y) as the reference returns them.
 * The transforms run in double through line plans that keep a (padded) line in the 64 KB of LDS a workgroup may take: powers of two up
 * to 4096 samples per side, other sizes (Bluestein, padded to the next power of two above 2 n) up to ~2048; larger sides fail with
 * XH_ERR_UNSUPPORTED at create (the typed tests of the reference stop at 768). */
typedef struct xh_shiftcorr xh_shiftcorr;
int xh_shiftcorr_create(xh_ctx *ctx, int32_t xdim, int32_t ydim, int32_t max_shift, xh_shiftcorr **out);
int xh_shiftcorr_destroy(xh_shiftcorr *h);
int xh_shiftcorr_load_reference(xh_shiftcorr *h, const float *d_ref);
int xh_shiftcorr_correlate(xh_ctx *ctx, float *d_inout, const float *d_ref, int32_t n, int32_t fy, int32_t fx, int32_t center);
int xh_shiftcorr_compute_shifts(xh_shiftcorr *h, const float *d_others, int32_t n, float *h_shifts);
/* Alignment::PolarRotationEstimator<T>, AlignType::OneToN (reconstruction/polar_rotation_estimator.cpp:33-144): d_ref [D][D], d_others
 * [n][D][D] -> h_rotations [n] degrees as getRotations2D returns them (an image rotated by a reads 360 - a). The reference's own
 * arithmetic: rings sampled with BsplineOrder 1 (bilinear, zero outside), not normalised, correlation over 2 N - 1 angles
 * (polar_rotation_estimator.cpp:58-60,94-99), double precision, the first maximum (data/polar.cpp:212-233). */
int xh_rotation_estimate(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t D, int32_t first_ring, int32_t last_ring,
                         float *h_rotations);
/* BSplineGeoTransformer<T>::interpolate (reconstruction/bspline_geo_transformer.cpp:103-137): d_dst[i] = applyGeometry(LINEAR, d_src[i],
 * h_matrices[i] (3 x 3 row major), IS_INV, DONT_WRAP), outside value 0; d_src and d_dst [n][ydim][xdim], not aliased */
int xh_apply_geometry2d(xh_ctx *ctx, const float *d_src, int32_t n, int32_t ydim, int32_t xdim, const float *h_matrices, float *d_dst);
/* CorrelationComputer<T>, OneToN, normalised (reconstruction/correlation_computer.cpp:30-56): h_merit[i] = correlationIndex(ref, others[i]) */
int xh_correlation_merit(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t ydim, int32_t xdim, float *h_merit);
/* Alignment::IterativeAlignmentEstimator<T>::compute(others, iters) (reconstruction/iterative_alignment_estimator.cpp:96-176) over the three
 * estimators above: rotation -> shift and shift -> rotation, `iters` rounds each, the images re-interpolated from the originals by the
 * inverse pose after every step; per image the order with the better merit. h_poses [n][9], h_merit [n]. */
int xh_iterative_alignment(xh_ctx *ctx, const float *d_ref, const float *d_others, int32_t n, int32_t D, int32_t max_shift, int32_t first_ring,
                           int32_t last_ring, int32_t iters, float *h_poses, float *h_merit);

/* ---- xmipp_align_significant (reconstruction/aalign_significant.cpp, reconstruction_adapt_cuda/align_significant_gpu.cpp) ----
 * Every (reference, image) pair aligned with the chain of xh_iterative_alignment, computed for batches of pairs, pair g = r N + i.
 * The references' polar transforms, shift spectra and pixels are prepared once per load; every step's pose algebra (the rotation2DMatrix
 * product, the shift add, M3x3_INV with its double reciprocal) runs on the device. Same arithmetic as xh_iterative_alignment: the two
 * agree pair for pair.
 * create: images of D x D pixels (even), up to max_refs references loaded at a time (<= 65535; per-reference buffers of about 22 bytes per
 * pixel are kept for them, none for the images, which may be any number), batch_pairs pairs per batch (<= 65535; the work space is
 * about 600 KB per pair at D = 128), max_shift < D / 2. The CUDA program's settings (align_significant_gpu.cpp:315-375) are max_shift
 * = D / 4, the default rings (first max(2, D / 20), last (D - 3) / 2) and iters = 3. */
typedef struct xh_align_sig xh_align_sig;
int xh_align_sig_create(xh_ctx *ctx, int32_t D, int32_t max_refs, int32_t batch_pairs, int32_t max_shift, int32_t first_ring, int32_t last_ring,
                        int32_t iters, xh_align_sig **out);
int xh_align_sig_destroy(xh_align_sig *h);
/* d_refs [R][D][D] on the device, R <= max_refs; replaces the references loaded before */
int xh_align_sig_load_references(xh_align_sig *h, const float *d_refs, int32_t R);
/* d_images [N][D][D] against the R loaded references -> d_poses [R][N][9] (3 x 3 float, row major) and d_merit [R][N], device memory */
int xh_align_sig_align(xh_align_sig *h, const float *d_images, int32_t N, float *d_poses, float *d_merit);
/* computeWeightsAndSave (aalign_significant.cpp:233-311) on the device: d_merit [R][N] -> d_weights [R][N]. Reference r takes the merits of
 * every reference q with r == q or Euler_distanceBetweenAngleSets(rot_r, tilt_r, 0, rot_q, tilt_q, 0, true) <= ang_distance (degrees
 * between the projection directions); c = the rank of merit (r, s) in ascending order among those count N values; weight = merit /
 * maxMerit . c / (count N - 1) in float if merit > 0, else 0. Equal merits are ranked by (reference, image) index, as a stable sort of
 * the list the reference builds would rank them (std::sort leaves their order unspecified).
 * Deviation: where count N is 1 (one image, a reference that selects only itself) the reference computes c / 0 = NaN; the weight is 0.
 * Cost: every weight counts over all count N merits, O(count N^2) comparisons per reference (tools/bench_align_sig.py times it). */
int xh_align_sig_weights(xh_align_sig *h, const float *h_rot, const float *h_tilt, double ang_distance, const float *d_merit, int32_t R, int32_t N,
                         float *d_weights);
/* updateRefs (align_significant_gpu.cpp:174-287, aalign_significant.cpp:470-573): for each of R references r (none need to be loaded;
 * R <= 65535), the sum over its assignments k (h_ref_idx[k] == r) of h_weight[k] times image h_img_idx[k] of d_images [N][D][D] interpolated by the inverse (M3x3_INV)
 * of its pose h_pose[k] (3 x 3, LINEAR, outside 0), divided by a normaliser -> d_out_refs [R][D][D].
 * Cumulative normaliser: as the reference program, which declares its norm before the loop over references, reference r is divided by
 * the running sum of the weights of references 0 .. r in index order, not by its own sum.
 * Deviation: a reference without assignments is zeros (the reference's memset), and so is any reference whose running sum is still 0,
 * where the reference program would divide 0 by 0 and write NaN. */
int xh_align_sig_update_refs(xh_align_sig *h, const float *d_images, int32_t N, int32_t R, int32_t n_assign, const int32_t *h_ref_idx,
                             const int32_t *h_img_idx, const float *h_weight, const float *h_pose, float *d_out_refs);

/* ---- xmipp_reconstruct_significant (reconstruction/reconstruct_significant.cpp) ----
 * alignImagesConsideringMirrors (data/filters.cpp:2047-2178) of every (image, gallery projection) pair in double precision, the imed of
 * every pair, and the program's two significance weightings. A chain is one (pair, mirror, order) triple, order 0 = shift then rotate,
 * 1 = rotate then shift; chain c = (pair . mirrors + mirror) . 2 + order, pair = image . G + projection. Per step only the chains whose
 * last increment is over the thresholds (0.95 px, 1 degree; :2072-2110) run, through a list compacted on the device.
 * create: images of D x D pixels (D even, >= 16, lines that fit the double-precision transform), up to max_gallery projections, batch_chains
 * chains per batch (1 .. 65532; a batch holds whole pairs, so at least 4; about 24 D^2 + 1 KB bytes of work space per chain). */
typedef struct xh_rsig xh_rsig;
int xh_rsig_create(xh_ctx *ctx, int32_t D, int32_t max_gallery, int32_t batch_chains, xh_rsig **out);
int xh_rsig_destroy(xh_rsig *h);
/* computeAlignmentTransforms (filters.cpp:2035-2040) of d_gallery [G][D][D] (doubles, G = volumes . directions <= max_gallery), once: the
 * forward transform as FourierTransformer leaves it (divided by D^2) and polarFourierTransform<true>(.., not conjugated, D / 5, D / 2,
 * BsplineOrder 1) (polar.cpp:152-176): bilinear samples at the float angle cache's coordinates, zero outside, normalised by
 * computeAverageAndStddev / normalize (polar.h:488-546), every ring's DFT / nsam. Replaces the gallery loaded before. */
int xh_rsig_load_gallery(xh_rsig *h, const double *d_gallery, int32_t G);
/* alignImagesToGallery's inner loop (reconstruct_significant.cpp:198-221) for d_images [N][D][D] (doubles, Xmipp origin) against the
 * loaded gallery. check_mirrors != 0: alignImagesConsideringMirrors (filters.cpp:2150-2178; the mirror is selfReverseX, and M(0,0),
 * M(1,0) are negated where it wins on corrMirror > corr); 0: alignImages alone (:211). Each is alignImages (:2047-2129): three rounds of
 * bestNonwrappingShift (:1903-1985; bestShift without mask or limit, then the three answers a period away, each on a strict > against the
 * first) and best_rotation over 2 N - 1 angles, in both orders, the image re-interpolated from the original (applyGeometry LINEAR,
 * IS_NOT_INV, DONT_WRAP) after every step, a step skipped once its last increment is within +-0.95 px on both axes / not above 1 degree
 * (initially 1.95 px, 2 degrees), corrRS > corrSR at the end.
 * Device outputs: d_M [N][G][9] as alignImagesConsideringMirrors returns it (before the program's M.inv()), d_corr [N][G], d_imed [N][G]
 * (imedDistance of the projection and the winning aligned image, filters.cpp:1269-1318, weights from their formula), and, nullable,
 * d_trace [N][G]: bit 0 the mirror won, bit 1 RS won, bits 2 .. 10 the winning mirror's SR chain, bits 11 .. 19 its RS chain, a chain's nine
 * bits being, for round r = 0 .. 2, 3 r: the shift step ran, 3 r + 1: the rotation step ran, 3 r + 2: a non-wrapping alternative replaced
 * bestShift's answer. The four d_chain_* (all or none): every chain's matrix [chains][9], correlation, imed and nine trace bits.
 * Deviation: applyGeometry's source coordinate of pixel (i, j) is x A00 + y A01 + A02 computed directly, where xmippCore adds A00 along the row. */
int xh_rsig_align(xh_rsig *h, const double *d_images, int32_t N, int32_t check_mirrors, double *d_M, double *d_corr, double *d_imed, int32_t *d_trace,
                  double *d_chain_M, double *d_chain_corr, double *d_chain_imed, int32_t *d_chain_trace);
/* The weights of reconstruct_significant.cpp:222-226 + :288-369 (per image) and :439-492 (per direction) on device arrays [N][G],
 * G = n_vols . n_dirs, direction g of angles h_rot [G], h_tilt [G] (degrees). one_alpha = 1 - alpha - deltaAlpha2.
 * First, with max_shift > 0, a pair whose shift (transformationMatrix2Parameters2D of M.inv()) exceeds it on either axis gets corr / 3
 * and imed . 3, IN PLACE in d_cc and d_imed. Per image: bestCorr, bestImed, ccl = tanh(atanh(bestCorr one_alpha) - 2.96 / sqrt(D^2)), the
 * cdfs of cc and imed over its G values; a pair is selected when ((apply_fisher && cc >= ccl) || !apply_fisher) && cdfcc >= one_alpha and
 * its shift is within max_shift; its weight is cdfcc (cc / bestCorr), times (1 - cdfimed)(bestImed / imed) with use_imed; others 0.
 * Per direction, as written in the reference: the neighbour loop re-reads the direction's own correlations, so the ranked list is its N
 * values repeated 1 + k times, k = the directions of the same volume sharply closer than ang_distance; weight *= cc (1 / bestCorr) cdf if
 * (cdf >= one_alpha || !strict) && weight > 0, else 0.
 * cdf (i) = (1-based ascending rank of element i) / n, equal values ranked by position (the first copy of a repeated value lowest);
 * ranks are counted, the repeated list is never built: rank = (1 + k) less (i) + equalBefore (i) + 1 of (1 + k) N. */
int xh_rsig_weights(xh_rsig *h, const double *d_M, double *d_cc, double *d_imed, int32_t N, int32_t n_vols, int32_t n_dirs, const double *h_rot,
                    const double *h_tilt, double ang_distance, double one_alpha, int32_t apply_fisher, int32_t use_imed, int32_t strict, double max_shift,
                    double *d_weight);
/* h_stats [13]: of the last align, the steps launched, the chains that ran the shift step in rounds 1, 2, 3, the chains that ran the
 * rotation step in rounds 1, 2, 3, its device seconds; of the last weights, the seconds of the per-image and the per-direction stage; of
 * the last align again, the device seconds inside shift steps and inside rotation steps, 0 unless the run was timed; of the last weights,
 * the host seconds of counting every direction's neighbours (n_vols n_dirs^2 angles, before any device work) */
int xh_rsig_stats(const xh_rsig *h, double *h_stats);
/* on: align puts events around every step and waits for each (one more synchronisation per step); for measurements */
int xh_rsig_set_timing(xh_rsig *h, int32_t on);

/* ---- xmipp_volume_halves_restoration (reconstruction_cuda/cuda_volume_halves_restorator.cpp, cuda_volume_restoration_kernels.cpp,
 * cuda_cdf.cpp; CPU counterpart reconstruction/volume_halves_restoration.cpp) ----
 * Two half maps [Z][Y][X] (fp64, any size up to 1024 per axis, X >= 2) restored in place by the reference's four stages, in the order of
 * VolumeHalvesRestorator::apply: denoise, deconvolve, filter_bank, difference. A stage given 0 iterations (filter bank: step 0) does
 * nothing and leaves its output absent. create sizes every buffer once (13 volumes' worth); the stages allocate nothing.
 * Masks are int32 [Z][Y][X] on the device, nonzero = inside. Inputs must be finite.
 * Deviations from the reference (each where it divides 0 by 0, reads out of bounds or does not terminate; details in xh_halves.hip):
 * a weight of 0 where the difference's standard deviation is 0, where weightFun 2 has w1 + w2 = 0, and for weightFun 3; the true half
 * spectrum size Z Y (X/2 + 1) where the reference uses X Y (Z/2 + 1); CDF ranks clamped to N - 1; an empty mask and a filter step
 * (1 - overlap) <= 0 refused with XH_ERR_ARG. Like the reference, weightPower is truncated to an integer. */
typedef struct xh_halves xh_halves;
int xh_halves_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_halves **out);
int xh_halves_destroy(xh_halves *h);
/* copies the two half maps into the handle; every output but the two restored volumes becomes absent */
int xh_halves_load(xh_halves *h, const double *d_v1, const double *d_v2);
/* denoise (significanceRealSpace); d_mask may be null */
int xh_halves_denoise(xh_halves *h, int32_t iters, const int32_t *d_mask);
/* deconvolution: sigmas searched on the host by Powell (xmipp3_amd/host/powell.h, ftol 0.01) over the device cost; h_sigmas (nullable)
 * receives the (sigma1, sigma2) of each iteration, 2 iters values. Outputs deconvolved and convolved. Synchronous. */
int xh_halves_deconvolve(xh_halves *h, int32_t iters, double sigma0, double lambda, double *h_sigmas);
/* filter bank; weightFun 0 mean, 1 min, 2 mean*diff, 3 (weight 0). Output filterBank. */
int xh_halves_filter_bank(xh_halves *h, double step, double overlap, int32_t weightFun, double weightPower);
/* difference; d_mask may be null. Output avgDiff. Synchronous. */
int xh_halves_difference(xh_halves *h, int32_t iters, double K, const int32_t *d_mask);
/* which: 0 restored1, 1 restored2, 2 filterBank, 3 deconvolved, 4 convolved, 5 avgDiff. *present = whether its stage ran; if it did and
 * d_out is not null, the volume is copied to d_out [Z][Y][X] */
int xh_halves_output(xh_halves *h, int32_t which, double *d_out, int32_t *present);
/* one deconvolution iteration's spectra from the current volumes (estimateS, then fft of S, V1, V2), and restorationSigmaCost's error
 * on them (synchronous): the pieces of xh_halves_deconvolve, exposed for tests */
int xh_halves_deconv_spectra(xh_halves *h);
int xh_halves_sigma_cost(xh_halves *h, double sigma1, double sigma2, double *h_cost);
/* the handle's 3-D transforms: r2c d_in [Z][Y][X] -> d_out [Z][Y][X/2+1] complex (interleaved doubles), un-normalised; c2r back, times
 * scale (d_in is not modified) */
int xh_halves_fft_r2c(xh_halves *h, const double *d_in, void *d_out);
int xh_halves_fft_c2r(xh_halves *h, const void *d_in, double *d_out, double scale);
/* Gpu::CDF: keys d_a^2 (d_b null) or mult (d_a - d_b)^2 over the voxels of d_mask (null: all) -> h_table [202]: the minimum, the 200 order
 * statistics of ranks round(p N) (N - 1 at most), p = 0.0025, 0.0075, ... as the reference's float loop makes them, the maximum.
 * Synchronous. */
int xh_halves_cdf(xh_halves *h, const double *d_a, const double *d_b, const int32_t *d_mask, double mult, double *h_table);
/* filter-bank timing (events around each band's transforms, CDF and weights; synchronises once per band when on) */
int xh_halves_set_timing(xh_halves *h, int32_t on);
int xh_halves_band_timing(xh_halves *h, int32_t *bands, double *h_ms);

/* host only, no device needed: the program's two mask types. circular: BinaryCircularMask about the Xmipp origin (index - size / 2)
 * shifted by (x0, y0, z0); R1 < 0 keeps r <= |R1|, R1 > 0 keeps r >= R1. binary: a mask file's values truncated to int, nonzero -> 1. */
int xh_halves_circular_mask(int32_t Z, int32_t Y, int32_t X, double R1, double x0, double y0, double z0, int32_t *h_mask);
int xh_halves_binary_mask(const float *h_values, size_t n, int32_t *h_mask);

/* Powell's direction-set minimiser of xmipp3_amd/host/powell.h (host only, no device needed): minimises f over p[0 .. n-1] starting with
 * the axis directions scaled by steps, stopping at a relative decrease below ftol. f reads the variables 1-based, x[1] .. x[n], as
 * xmippCore's powellOptimizer passes them. The minimum may differ from xmippCore's within ftol. */
typedef double (*xh_cost_fn)(double *x, void *user);
int xh_powell_minimize(int32_t n, double *p, const double *steps, double ftol, xh_cost_fn f, void *user, double *fret, int32_t *iter);

/* Many Powell searches in lockstep (xmipp3_amd/host/powell_batch.h; host only, no device needed): problem q minimises over its n[q]
 * variables p[q * nmax .. q * nmax + n[q] - 1] with the steps at the same places. Each search is xh_powell_minimize's own code paused at
 * every cost call; at each step the live searches' vectors (at most `capacity` of them, never a finished problem's) go to f in one call:
 * row r is problem[r] with its variables 0-based at x[r * nmax ..]; f writes cost[r] and returns 0 (anything else ends the run and is
 * returned). A finished search gives its slot to the next problem. Every problem's minimum, cost and iteration count are bit for bit
 * what xh_powell_minimize gives for it alone; evals (nullable) receives the number of cost calls of each. */
typedef int32_t (*xh_batch_cost_fn)(int32_t m, const int32_t *problem, const double *x, double *cost, void *user);
int xh_powell_minimize_batch(int32_t nprob, const int32_t *n, int32_t nmax, double *p, const double *steps, double ftol, int32_t capacity,
                             xh_batch_cost_fn f, void *user, double *fret, int32_t *iter, int64_t *evals);

/* ---- xmipp_angular_continuous_assign2 (reconstruction/angular_continuous_assign2.cpp; CUDA twin
 * reconstruction_adapt_cuda/angular_continuous_assign2_gpu.cpp) ----
 * Continuous refinement of each particle's pose against projections of a volume: Powell's method over continuous2cost (L348-395).
 * The searches of all particles advance in lockstep, one cost evaluation of every live search per device step (xh_ca2.hip).
 * The 13 variables of a row are the reference's p(0..12): a, b (grey I' = a I + b), shift x, y (added to the input shift), scale x, y,
 * scale angle, change of rot, tilt, psi, change of defocus U, V, defocus angle.
 * A particle with a CTF has its projections multiplied by generateCTF's image at K = 1 (updateCTFImage L225-247: the CTF with its damping
 * envelope; its absolute value when phase_flipped) and its spectrum by the envelope image (L447-460); the CTF's noise model is not read.
 * Refused with XH_ERR_UNSUPPORTED: particles of another size than the volume (scaleToSize, L574-578). */
typedef struct xh_ca2 xh_ca2;
typedef struct {
    double max_shift, max_scale, max_angular_change, max_defocus_change, max_resolution, max_gray_scale, max_gray_shift, sampling, Rmax,
        padding;                                                                                     /* readParams L52-62 */
    int32_t optimize_gray, optimize_shift, optimize_scale, optimize_angles, optimize_defocus, phase_flipped, same_defocus;
} xh_ca2_params;
/* one particle's input row (processImage L421-445): the caller resolves the continuous* columns (continuousX / Y / Flip replace
 * shiftX / Y / flip when continuousScaleX is present) */
typedef struct {
    double rot, tilt, psi, shift_x, shift_y, scale_x, scale_y, scale_angle, gray_a, gray_b;
    int32_t flip, has_ctf;
    xh_ctf_params ctf;      /* read when has_ctf: the row's CTF (readFromMdRow); phase_shift in degrees; K is taken as 1 (updateCTFImage) */
} xh_ca2_row;
/* the program's defaults (defineParams L121-140) */
void xh_ca2_defaults(xh_ca2_params *p);
/* preProcess (L157-222): the projector FourierProjector(V, padding, sampling / max_resolution, BSPLINE3) through xh_fp_create, the binary
 * circular mask of radius Rmax (< 0: D / 2), the cost type (L1 when grey values are optimised, else minus the masked correlation).
 * The random covariance of L189-201 feeds nothing and is not built. capacity: evaluations per device step. */
int xh_ca2_create(xh_ctx *ctx, const float *d_vol, int32_t D, const xh_ca2_params *prm, int32_t capacity, xh_ca2 **out);
int xh_ca2_destroy(xh_ca2 *h);
/* processImage L414-478 for n particles h_images [n][ydim][xdim] (host): Istddev, Ifiltered = the raised-cosine low pass at
 * sampling / max_resolution, raised_w 0.02 (fourier_filter.cpp:423-432, 710-716), times the CTF envelope where the particle has a CTF
 * (generateEnvelope, ctf.h:1271-1290), resident as doubles; replaces what was loaded */
int xh_ca2_load(xh_ca2 *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_ca2_row *rows);
/* continuous2cost + tranformImage (L251-395) of m rows: particle h_particle[r] at the 13 variables h_vars[r][13] -> h_cost[r]. A row
 * outside the bounds of L364-375, or with a non-finite variable, costs 1e38 and no device work. Where a variance under the mask is 0 the correlation is 0.
 * A row's cost does not depend on the rows it is evaluated with. Synchronous. */
int xh_ca2_cost(xh_ca2 *h, int32_t m, const int32_t *h_particle, const double *h_vars, double *h_cost);
/* P (the projection), E (the residual) and Ifilteredp (the transformed particle, 0 outside the mask) [D][D] doubles of device row `row`
 * of the last evaluation (the in-bound rows of the last xh_ca2_cost chunk, in order); null pointers are skipped.
 * Deviation: the reference writes these from whatever Powell evaluated last, which is generally not the minimum it returns; here the
 * caller evaluates once more at the returned variables (xh_ca2_cost) and reads them then. */
int xh_ca2_last_images(xh_ca2 *h, int32_t row, double *d_P, double *d_E, double *d_Ifilteredp);
/* the similarity measures of processImage (L543-547) between P and Ifilteredp of device row `row` of the last evaluation -> h_out[3]:
 * corrIdx (correlationIndex without mask), corrMask (correlationMasked, filters.cpp:1397-1452; 0 where the reference divides 0 by 0),
 * imed (imedDistance, filters.cpp:1269-1318, its 7 x 7 weights exp(-(x^2 + y^2) / 2) / sqrt(2 pi) from the formula). Computed on the host
 * from the two images (once per particle, sequential sums in the reference's order). corrWeight (correlationWeighted, which needs
 * alignImages) is not computed. */
int xh_ca2_measures(xh_ca2 *h, int32_t row, double *h_out);
/* the final transform of processImage (L571-613) for every loaded particle: h_images [n][D][D] (host; the --applyTo images, in the order
 * loaded) through applyGeometry(BSPLINE3, ., A, IS_NOT_INV, DONT_WRAP) with A of L579-598 at h_vars [n][13], then (I - b) / a inside the
 * mask and 0 outside when grey values were optimised (L600-612) -> h_out [n][D][D] float. Synchronous. */
int xh_ca2_apply(xh_ca2 *h, const float *h_images, const double *h_vars, float *h_out);
/* Ifiltered [D][D] (host, nullable) and Istddev (nullable) of a loaded particle */
int xh_ca2_filtered(xh_ca2 *h, int32_t particle, double *h_out, double *h_stddev);
/* the search of processImage (L488-540) for every loaded particle, ftol 0.01: h_vars [n][13], h_cost [n] (Powell's minimum: minus the
 * correlation, or the L1 cost), h_iter [n], h_evals [n] (cost calls, those the bounds decided included), h_enabled [n] (1, or -1: the
 * input scale out of bounds L489-491, where cost is -1 and nothing is searched; a search ending on the 1e38 barrier or at a positive
 * correlation cost L523-540, where the variables return to their input values).
 * Only the variables whose step is non-zero are searched (the reference hands Powell all 13, the frozen ones with step 0, and spends
 * line searches on flat directions): results agree with the reference within ftol, not bit for bit. */
int xh_ca2_refine(xh_ca2 *h, double *h_vars, double *h_cost, int32_t *h_iter, int64_t *h_evals, int32_t *h_enabled);
/* of the last refine: device steps, rows evaluated, seconds inside device steps (upload to the wait's end), seconds in all */
int xh_ca2_stats(const xh_ca2 *h, double *h_stats);

/* ---- xmipp_volume_deform_sph (reconstruction/volume_deform_sph.cpp; CUDA twin reconstruction_adapt_cuda/volume_deform_sph_gpu.cpp,
 * reconstruction_cuda/cuda_volume_deform_sph.cu) ----
 * The Zernike3D deformation that fits an input volume to a reference: g(p) = sum_idx c_idx Z_idx(p / Rmax) inside the ball r < Rmax about
 * the Xmipp origin (index - size / 2), 0 outside, fitted by Powell's method over
 *   cost = sqrt(diff2 / count) + lambda (sqrt(modg / count) + |sumVI - sumVD| / sumVI)
 * with, over every voxel of every (input I_p, reference R_p) pair, vI = I_p sampled trilinearly at p + g(p) (0 outside the volume),
 * diff2 = sum (R_p - vI)^2, sumVD = sum of the vI >= 0, modg = sum |g|^2, count = pairs Z Y X, sumVI = sum of the input voxels >= 0.
 * Everything is fp64; the volumes stay on the device. Volumes and results of these calls are host arrays [Z][Y][X].
 * The variables x [3 nterms] are cx, then cy, then cz of every term, in the order of xh_vds_terms.
 * Supported degrees: l1 <= 5, l2 <= 4 (the polynomial forms); anything beyond is XH_ERR_UNSUPPORTED. Deviations from the reference
 * (details in xh_vds.hip): the displacement is the CUDA twin's (the CPU loop drops a term whose x coefficient is 0); the search moves
 * only the variables whose step is 1; normalize_Robust follows stated readings of xmippCore primitives. */
typedef struct xh_vds xh_vds;
/* host only, no device needed. Terms of degrees (L1, L2) (numCoefficients): for h = 0 .. L2, l = h, h + 2, ... <= L1, m = -h .. h the term
 * (l1 = l, n = h, l2 = h, m), written to out [n][4] (fillVectorTerms) */
int xh_vds_num_terms(int32_t L1, int32_t L2, int32_t *n);
int xh_vds_terms(int32_t L1, int32_t L2, int32_t *out);
/* host only: one basis term, R_l1^n(r) S_l2^m(xr, yr, zr) (ZernikeSphericalHarmonics), by the function the kernels run */
int xh_vds_zsh(int32_t l1, int32_t n, int32_t l2, int32_t m, double xr, double yr, double zr, double r, double *out);
/* host only: normalize_Robust with a zero background mask, in place: (v - median of the background) / (99th percentile of the
 * foreground) with the two split by EntropySegmentation, clipped to +-clip when clip > 0 (the program: 1.3284). A constant volume, an
 * empty foreground or background and a percentile <= 0 are XH_ERR_ARG. */
int xh_vds_normalize_robust(double *v, size_t n, double clip);
/* Rmax < 0: X / 2 */
int xh_vds_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t L1, int32_t L2, double Rmax, double lambda, xh_vds **out);
int xh_vds_destroy(xh_vds *h);
/* Rmax as resolved, the number of terms, sumVI of the loaded pairs; null pointers are skipped */
int xh_vds_info(const xh_vds *h, double *Rmax, int32_t *nterms, double *sumVI);
/* REALGAUSSIAN low pass exp(-pi^2 w^2 sigma^2), w the digital frequency (FourierFilter::applyMaskSpace). Synchronous. */
int xh_vds_gauss(xh_vds *h, double sigma, const double *h_in, double *h_out);
/* the pairs h_I, h_R [npairs][Z][Y][X] (already normalised), copied to the device; computes sumVI and the share of diff2 and sumVD of
 * the voxels with r >= Rmax, which no coefficient changes */
int xh_vds_set_pairs(xh_vds *h, int32_t npairs, const double *h_I, const double *h_R);
/* one evaluation at h_x [3 nterms] -> h_out[4] = cost, diff2, sumVD, modg. The same h_x gives the same bits on every call. Synchronous. */
int xh_vds_cost(xh_vds *h, const double *h_x, double *h_out);
/* one stage of the program's loop: Powell (xh_powell_minimize, ftol 0.01) from h_x over the first numCoefficients(L1, l2_stage) entries
 * of each third of h_x, step 1; the others stay. fret is the cost at the returned h_x; evals (nullable) the number of evaluations. */
int xh_vds_refine_stage(xh_vds *h, int32_t l2_stage, double *h_x, double *fret, int32_t *iter, int64_t *evals);
/* h_VO = h_raw sampled at p + g(p); h_G (nullable) [3][Z][Y][X] = gx, gy, gz, exactly 0 where r >= Rmax. Synchronous. */
int xh_vds_apply(xh_vds *h, const double *h_raw, const double *h_x, double *h_VO, double *h_G);
/* computeStrain: h_G [3][Z][Y][X] is low-passed (REALGAUSSIAN, sigma 2) in place; over the interior (2 voxels in from every face), with
 * U = grad g by the five-point stencil (1, -8, 8, -1) / 12, h_LS = |det(sym U)| and h_LR = 180 / pi sqrt(h01^2 + h02^2 + h12^2) of the
 * antisymmetric part (the modulus of its imaginary eigenvalues) where that exceeds 1e-6, else 0; both are 0 on the border. Synchronous. */
int xh_vds_strain(xh_vds *h, double *h_G, double *h_LS, double *h_LR);

/* ---- xmipp_angular_sph_alignment (reconstruction/angular_sph_alignment.cpp; CUDA twin
 * reconstruction_adapt_cuda/angular_sph_alignment_gpu.cpp, reconstruction_cuda/cuda_angular_sph_alignment.cu) ----
 * For every particle a pose and a Zernike3D deformation of the reference volume, fitted by Powell's method over
 *   cost = -correlationIndex(Ifilteredp, P, mask2D) + lambda (sqrt(modg / count) + |sumV - sumVd| / sumV)
 * with P the projection along z of the volume sampled at R^-1 p + g(R^-1 p), R = Euler(rot, tilt, psi), over the voxels with r < RDef
 * whose displaced position falls on a mask voxel equal to 1 (deformVol L530-609), then multiplied by the particle's CTF and low-passed.
 * The nvars = 3 vecSize + 8 variables of a row are the reference's p: cx, cy, cz of every term (the order of xh_vds_terms), then the change
 * of shift x, y, of rot, tilt, psi, of defocus U, V and of the defocus angle. Everything is fp64; the searches of all loaded particles
 * advance in lockstep, one evaluation of every live search per device step. A row's results never depend on the rows evaluated with it.
 * Deviations from the reference are listed at the head of xmipp3_amd/csrc/xh_asa.hip. */
typedef struct xh_asa xh_asa;
typedef struct {
    double max_shift, max_angular_change, max_resolution, sampling, Rmax, RDef, lambda;      /* readParams L52-64; lambda: --regularization */
    int32_t l1, l2, optimize_alignment, optimize_deformation, optimize_defocus, phase_flipped;
} xh_asa_params;
/* one particle's input row (processImage L304-325) */
typedef struct {
    double rot, tilt, psi, shift_x, shift_y;
    int32_t flip, has_ctf;
    xh_ctf_params ctf;      /* read when has_ctf (readFromMdRow); phase_shift in degrees; K is taken as 1 (updateCTFImage L521-528) */
} xh_asa_row;
/* the program's defaults (defineParams L104-120) */
void xh_asa_defaults(xh_asa_params *p);
/* the flags of xh_asa_stage_active: --optimizeDeformation, --optimizeAlignment, --optimizeDefocus */
enum { XH_ASA_OPT_DEFORMATION = 1, XH_ASA_OPT_ALIGNMENT = 2, XH_ASA_OPT_DEFOCUS = 4 };
/* host only, no device needed: the indices (ascending, into the nvars variables of degrees (L1, L2)) of the variables that stage `stage`
 * (0 .. L2; the program runs 1 .. L2) frees: minimizepos (L472-482) and the steps of processImage (L351-358). out holds up to nvars. */
int xh_asa_stage_active(int32_t L1, int32_t L2, int32_t stage, int32_t flags, int32_t *out, int32_t *n);
/* preProcess (L125-188): d_vol [D][D][D] float (device) is kept as doubles; h_mask [D][D][D] int32 (host; null: the sphere of radius RDef);
 * sumV = the sum of the volume where the mask is 1 (0 or non-finite: XH_ERR_ARG); mask2D of radius Rmax; RDef, Rmax < 0: D / 2.
 * Degrees above l1 = 5, l2 = 4 are XH_ERR_UNSUPPORTED. capacity: evaluations per device step. */
int xh_asa_create(xh_ctx *ctx, const float *d_vol, int32_t D, const int32_t *h_mask, const xh_asa_params *prm, int32_t capacity, xh_asa **out);
int xh_asa_destroy(xh_asa *h);
/* RDef and Rmax as resolved, vecSize, the number of variables, sumV; null pointers are skipped */
int xh_asa_info(const xh_asa *h, double *RDef, double *Rmax, int32_t *vecSize, int32_t *nvars, double *sumV);
/* processImage L304-333 for n particles h_images [n][ydim][xdim] (host): Ifiltered = the raised-cosine low pass at sampling / max_resolution,
 * raised_w 0.02, resident as doubles; replaces what was loaded. Particles of another size than the volume: XH_ERR_UNSUPPORTED. */
int xh_asa_load(xh_asa *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_asa_row *rows);
/* continuousSphCost + tranformImageSph (L196-289) of m rows: particle h_particle[r] at the variables h_vars[r][nvars] -> h_cost[r]. A row
 * outside the bounds of L275-278, or with a non-finite variable, costs 1e38 and no device work; so does a row whose count is 0.
 * Synchronous. */
int xh_asa_cost(xh_asa *h, int32_t m, const int32_t *h_particle, const double *h_vars, double *h_cost);
/* of device row `row` of the last evaluation (the in-bound rows of the last chunk, in order): the projection before (d_P_raw) and after
 * (d_P) the CTF and the low pass, the transformed particle (d_Ifilteredp, 0 outside mask2D), [D][D] doubles on the device, and
 * h_sums[4] = sumVd, modg, count, corr (host); null pointers are skipped */
int xh_asa_last(xh_asa *h, int32_t row, double *d_P_raw, double *d_P, double *d_Ifilteredp, double *h_sums);
/* the search of processImage (L335-415) for every loaded particle: stages h = 1 .. l2, each Powell (ftol 0.01, step 1) over the variables
 * xh_asa_stage_active names, from the variables the stage before left; a stage that ends at a positive cost disables the particle and
 * zeroes its variables (L369-373). h_vars [n][nvars], h_cost [n] (the last stage's minimum: minus the correlation written), h_enabled [n]
 * (1 or -1), h_deformation [n] (sqrt(modg / count) of one more evaluation at the returned variables; 0 when that row is out of bounds),
 * h_iter [n] and h_evals [n] (iterations and cost calls over all stages). */
int xh_asa_refine(xh_asa *h, double *h_vars, double *h_cost, int32_t *h_enabled, double *h_deformation, int32_t *h_iter, int64_t *h_evals);
/* of the last xh_asa_cost or xh_asa_refine: device steps, rows evaluated on the device, seconds inside device steps, seconds in all */
int xh_asa_stats(const xh_asa *h, double *h_stats);

/* ---- xmipp_forward_art_zernike3d (reconstruction_adapt_cuda11/forward_art_zernike3d_gpu.cpp, reconstruction_cuda11/
 * cuda_forward_art_zernike3d.{cpp,cu}) ----
 * ART reconstruction of the undeformed volume from particles that each carry a pose and a Zernike3D deformation: per image the volume
 * is splatted through the image's field onto P and W planes (one pair per sigma), the planes are Gaussian-filtered, the residual against
 * the shifted (and CTF-inverted) particle is formed, and the residual is spread back along the same field, plus a regulariser. The
 * volume and the regulariser's four fields stay on the device over the whole run; a sweep over many images is one stream of kernels.
 * Everything is fp64. The contract and the deviations from the reference are at the head of xmipp3_amd/csrc/xh_faz.hip. */
typedef struct xh_faz xh_faz;
typedef struct {
    double RDef, sampling, lambda, ltv, ltk, ll1, lst;      /* --RDef, --sampling, --regularization, --ltv, --ltk, --ll1, --lst */
    int32_t l1, l2, step, use_zernike, use_ctf, phase_flipped;
} xh_faz_params;
/* one particle's input row (processImage :401-431) */
typedef struct {
    double rot, tilt, psi, shift_x, shift_y;
    int32_t flip, has_ctf;
    xh_ctf_params ctf;      /* read when has_ctf and use_ctf (readFromMdRow); Tm is replaced by --sampling */
} xh_faz_row;
/* the program's defaults (defineParams :132-168) */
void xh_faz_defaults(xh_faz_params *p);
/* host only: sortOrthogonal (:628-690) over n projection directions (rot, tilt in degrees); sort_last = --sort_last (-1: all). order [n] */
int xh_faz_sort_orthogonal(int32_t n, const double *h_rot, const double *h_tilt, int32_t sort_last, int32_t *h_order);
/* host only: the schedule of --save_iter over one iteration of n images (:587-592): h_flags[k] = 1 when the partial volume is written
 * after the k-th image */
int xh_faz_save_schedule(int32_t n, int32_t save_iter, int32_t *h_flags);
/* host only: the checks a program makes before it touches a device: the degrees, and the length of a coefficient vector against
 * 3 vecSize (ncoef < 0: not checked) */
int xh_faz_check(int32_t l1, int32_t l2, int32_t ncoef);
/* preProcess (:175-380). D: the side of the volume and of the images (<= 1024). h_V0 [D][D][D] doubles (host; null: zeros). h_maskF /
 * h_maskB [D][D][D] int32 (host): a mask read from a file, set to 0 here where k^2 + i^2 + j^2 >= RDef^2; null: the sphere
 * k^2 + i^2 + j^2 <= RDef^2. h_sigma [nsigma] (1 .. 8). h_sym [nsym][9] (nullable, nsym 0): the right matrices of the symmetry group
 * without the identity; every image is then presented once per matrix, the identity first, with the rotation E R_sym. */
int xh_faz_create(xh_ctx *ctx, int32_t D, const double *h_V0, const int32_t *h_maskF, const int32_t *h_maskB, const double *h_sigma,
                  int32_t nsigma, const double *h_sym, int32_t nsym, const xh_faz_params *prm, xh_faz **out);
int xh_faz_destroy(xh_faz *h);
/* RDef as resolved, vecSize, the bricks of the forward list, the presentations per image (1 + nsym); null pointers are skipped */
int xh_faz_info(const xh_faz *h, double *RDef, int32_t *vecSize, int32_t *nbricks, int32_t *per_image);
/* n particles h_images [n][ydim][xdim] (host) with their rows and, with use_zernike, their coefficients h_coef [n][3 vecSize] (cx of every
 * term, then cy, then cz: the sphCoefficients vector); replaces what was loaded. Step 4 of the contract (CTF inversion, shift and flip)
 * runs here for all of them. */
int xh_faz_load(xh_faz *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_faz_row *rows, const double *h_coef);
/* steps 2-7 for the loaded images first .. first + count - 1 in order, every presentation of an image in turn, without a host
 * synchronisation in between; h_errors [count][per_image]: sqrt(sum diff^2 / N) of every presentation (NaN when no pixel has weight) */
int xh_faz_sweep(xh_faz *h, int32_t first, int32_t count, double *h_errors);
/* steps 2-5 for presentation `sym` (0: the identity) of loaded image `index` against the current volume, which is not updated. Device
 * outputs, doubles, null pointers skipped: raw and filtered P and W [nsigma][D][D], Idiff, Iws and the prepared particle [D][D]. */
int xh_faz_forward(xh_faz *h, int32_t index, int32_t sym, double *d_P_raw, double *d_W_raw, double *d_P, double *d_W, double *d_Idiff,
                   double *d_Iws, double *d_particle, double *h_error);
/* the refined volume [D][D][D] doubles (host) */
int xh_faz_get_volume(xh_faz *h, double *h_V);
int xh_faz_set_volume(xh_faz *h, const double *h_V);
/* for the benchmark: with timing on, a sweep records events around its stages (they do not synchronise; the sweep still waits once, at
 * its end) and xh_faz_stage_ms returns the milliseconds of the last sweep, summed over its presentations: h_ms[5] = the splat (with the
 * clearing of the planes), the filter (conversion, two transforms, the multiply), the residual, the regulariser, the backward kernel */
int xh_faz_set_timing(xh_faz *h, int32_t on);
int xh_faz_stage_ms(const xh_faz *h, double *h_ms);

/* ---- projectVolume in real space: four rays per pixel through the voxel grid ------------------------
 * Replaces projectVolume(V, P, Ydim, Xdim, rot, tilt, psi, roffset) (libraries/data/projection.cpp:337-589), the projector that
 * xmipp_subtract_projection (reconstruction/subtract_projection.cpp:258,280,653) uses for its mask projections of every particle and,
 * with --realSpaceProjection, for the volume itself. fp64; the contract and the deviations are at the head of xmipp3_amd/csrc/xh_rsp.hip.
 *   create  : d_vol [D][D][D] doubles on the device, [z][y][x], Xmipp origin; it is read here and not kept. XH_RSP_VALUE: project()
 *             writes the line integrals (ray_sum * 0.25, L582). XH_RSP_SUPPORT: project() writes 1.0 where the line integral of a
 *             non-negative volume is positive and 0.0 elsewhere, from v > 0 packed into bits; a volume with a negative voxel takes the
 *             value walk followed by > 0 instead (xh_rsp_info's packed = 0).
 *   project : h_angles n x (rot, tilt, psi) degrees (Projection::setAngles, L345); h_offsets n x (x, y), the roffset subtracted from
 *             every ray's pixel coordinates (L412-413), or null (roffset == nullptr); d_out n x D x D doubles. Asynchronous on the
 *             context's stream. n = 0 does nothing.
 *   steps   : for the benchmark: the voxel steps the four rays of every pixel walk in the handle's mode (the bits end a ray at its
 *             first hit), d_steps n x D x D int32. */
typedef struct xh_rsp xh_rsp;
enum { XH_RSP_VALUE = 0, XH_RSP_SUPPORT = 1 };
int xh_rsp_create(xh_ctx *ctx, const double *d_vol, int32_t D, int32_t mode, xh_rsp **out);
int xh_rsp_destroy(xh_rsp *h);
int xh_rsp_info(const xh_rsp *h, int32_t *D, int32_t *mode, int32_t *packed);
int xh_rsp_project(xh_rsp *h, const double *h_angles, const double *h_offsets, int32_t n, double *d_out);
int xh_rsp_steps(xh_rsp *h, const double *h_angles, const double *h_offsets, int32_t n, int32_t *d_steps);

/* ---- xmipp_subtract_projection (libraries/reconstruction/subtract_projection.{h,cpp}) ----
 * Projects the refined volume at each particle's pose, fits the projection to the particle in Fourier space (order 0: T(w) = beta00,
 * order 1: T(w) = beta01 + beta1 w, the better adjusted R2 wins) and removes it, keeping or removing the region of a 3-D mask. The
 * reference runs one particle at a time on CPU threads; here `capacity` particles go through one stream of kernels per device step.
 * Everything is fp64. The contract and the deviations from the reference are at the head of xmipp3_amd/csrc/xh_sub.hip. */
typedef struct xh_sub xh_sub;
typedef struct {
    double sampling, max_resolution, padding, cirmaskrad;      /* --sampling, --max_resolution (-1: sampling), --padding, --cirmaskrad (-1: D / 2) */
    int32_t subtract, real_space, ignore_ctf, boost, non_negative, pad_;   /* --subtract, --realSpaceProjection, --ignoreCTF, --boost, --nonNegative */
} xh_sub_params;
/* one particle's input row (processParticle L246-252, applyCTF L219-225) */
typedef struct {
    double rot, tilt, psi, shift_x, shift_y;
    int32_t has_ctf, pad_;      /* has_ctf: the row holds ctfDefocusU */
    xh_ctf_params ctf;          /* read when has_ctf and not --ignoreCTF (readFromMdRow); Tm is replaced by --sampling, K comes from the row */
} xh_sub_row;
/* one particle's results (writeParticle L161-174): subtractionR2, subtractionBeta0, subtractionBeta1, subtractionB; model 0 or 1;
 * disable: --nonNegative and beta00 < 0; enabled: -1 when --nonNegative and (disable or R2adj < 0), else 1. beta00 and R20adj are the
 * order-0 figures whatever model won (for the tests). */
typedef struct {
    double R2adj, beta0, beta1, b, beta00, R20adj;
    int32_t model, disable, enabled, pad_;
} xh_sub_result;
/* the program's defaults (defineParams L116-151) */
void xh_sub_defaults(xh_sub_params *p);
/* host only: the integer frequency map wi [D][D/2+1] (L554-563; null: skipped) and maxwiIdx (L572-580) */
int xh_sub_freq_map(int32_t D, double sampling, double max_resolution, int32_t *h_wi, int32_t *maxwiIdx);
/* host only: the fit of L732-759 from the per-wi sums h_sums [maxwiIdx + 1][4] = num0, den0, sum (re + im) of PiMFourier, sum (re + im) of
 * IiMFourier, and a11 = sum 2 wi over the cells with 0 < wi < maxwiIdx: h_betas = beta00, beta01, beta1. solveLinearSystem is least squares
 * through the normal equations (parity with xmippCore unpinned: SURVEY.md Appendix B). The device runs this same code. */
int xh_sub_fit(const double *h_sums, int32_t maxwiIdx, double a11, double *h_betas);
/* host only: evaluateFitting for both models and checkBestModel (L323-364) from sum (re + im), sum (re^2 + im^2) of IFourier and the two
 * sums of squared errors over `cells` half-spectrum cells: h_out = R2adj of the chosen model, the model (0 when R21adj == R20adj), R20adj */
int xh_sub_choose(double sumY, double sumY2, double sumE0, double sumE1, double cells, double *h_out);
/* preProcess (L514-632). h_vol [D][D][D] doubles (host, Xmipp origin). h_roi: the --mask_roi volume or null (no ROI mask). h_maskvol: the
 * --mask volume or null (the 2-D disc of --cirmaskrad). capacity: particles per device step. */
int xh_sub_create(xh_ctx *ctx, const double *h_vol, int32_t D, const double *h_roi, const double *h_maskvol, const xh_sub_params *prm,
                  int32_t capacity, xh_sub **out);
int xh_sub_destroy(xh_sub *h);
/* maxwiIdx, the side of applyCTF's padded window, a11; null pointers are skipped */
int xh_sub_info(const xh_sub *h, int32_t *maxwiIdx, int32_t *padded, double *a11);
/* n particles h_images [n][ydim][xdim] (host) with their rows; replaces what was loaded. Non-square particles and particles of another size
 * than the volume: XH_ERR_UNSUPPORTED. */
int xh_sub_load(xh_sub *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_sub_row *rows);
/* processImage (L634-826) for every loaded particle, in chunks of `capacity`: h_out [n][D][D] doubles (Idiff), h_res [n] */
int xh_sub_run(xh_sub *h, double *h_out, xh_sub_result *h_res);
/* test hook: the planes of particle `index` of the last chunk, device doubles [D][D], null pointers skipped: P (the projection before the
 * CTF), Pctf (after it, before the mask), PmaskImg, M, iM, Idiff; on the host the sums [maxwiIdx + 1][4] of xh_sub_fit and its betas [3] */
int xh_sub_last(xh_sub *h, int32_t index, double *d_P, double *d_Pctf, double *d_PmaskImg, double *d_M, double *d_iM, double *d_Idiff,
                double *h_sums, double *h_betas);
/* for the benchmark: with timing on, a run records events around its stages (they do not synchronise; a chunk still waits once, at its
 * end) and xh_sub_stage_ms returns the milliseconds of the last run, summed over its chunks: h_ms[7] = the projection (with the
 * translation), the CTF (pad, two transforms, the multiply, the crop), the mask projections, b with the four spectra, the sums per wi with
 * the fit, the two models with the choice, the output (spectrum, inverse transform, difference) */
int xh_sub_set_timing(xh_sub *h, int32_t on);
int xh_sub_stage_ms(const xh_sub *h, double *h_ms);

/* ---- xmipp_resolution_monogenic_signal, MonoRes (libraries/reconstruction/resolution_monogenic_signal.{h,cpp}, the Monogenic class of
 * libraries/data/monogenic_signal.{h,cpp}) ----
 * The local resolution map of a volume (or of two half maps) by a sweep over frequencies: at each one the monogenic (Riesz) amplitude of
 * the high-passed map is compared, voxel by voxel, with a threshold taken from the noise. The reference runs on CPU threads; here the
 * whole sweep stays on the device and the host reads one small record per frequency. Everything is fp64. The kernels, the reference
 * behaviours kept as written and the deviations are listed at the head of xmipp3_amd/csrc/xh_mono.hip. Volumes are [Z][Y][X]. */
typedef struct xh_mono xh_mono;
typedef struct {
    double sampling, minRes, maxRes, freq_step, significance;   /* --sampling_rate, --minRes (overwritten by 2 sampling, run :362), --maxRes, --step, --significance */
    int32_t gaussian, noise_only_in_halves;                     /* --gaussian, --noiseonlyinhalves */
} xh_mono_params;
/* statisticsInBinaryMask2 / statisticsInOutBinaryMask2 (monogenic_signal.cpp :424-508) */
typedef struct {
    double NS, NN, sumS, sumS2, sumN, sumN2, meanS, sdS2, meanN, sdN2, thr95;
} xh_mono_stats;
/* one evaluated frequency of run (:392-536): threshold and z are 0 where the sweep left before computing them; assigned: the assign
 * kernel ran */
typedef struct {
    xh_mono_stats stats;
    double resolution, freq, freqH, freqL, threshold, z, max_meanS;
    int32_t assigned, pad_;
} xh_mono_step;
/* why the sweep ended: resolution2eval's break (:407), NS / NVoxelsOriginalMask < 0.025 (:460), NS == 0 (:481), meanS < 0.001 max_meanS
 * (:499), z < criticalZ (:525), resolution < minRes (:531) */
enum { XH_MONO_STOP_RANGE = 1, XH_MONO_STOP_MASK_DONE = 2, XH_MONO_STOP_NO_POINTS = 3, XH_MONO_STOP_LOW_SIGNAL = 4, XH_MONO_STOP_ZTEST = 5,
       XH_MONO_STOP_MIN_RES = 6 };
/* the program's defaults (defineParams :51-87) */
void xh_mono_defaults(xh_mono_params *p);
/* host only: icdf_gauss (xmippCore) restated as Abramowitz-Stegun 26.2.23 (parity unpinned) */
int xh_mono_icdf_gauss(double p, double *out);
/* host only: Monogenic::resolution2eval (monogenic_signal.cpp :212-272), state in and out as in the reference; a resolution <= 0 breaks */
int xh_mono_resolution2eval(int32_t *count_res, double step, double *resolution, double *last_resolution, double *freq, double *freqL,
                            int32_t *last_fourier_idx, int32_t volsize, int32_t *continueIter, int32_t *breakIter, double sampling, double maxRes);
/* host only: the shell walk of findCliffValue (:70-105) over per-shell sums (shell r: r^2 <= k^2 + i^2 + j^2 < (r + 1)^2) */
int xh_mono_cliff_radius(const double *h_sum, const double *h_sum2, const double *h_N, int32_t nshell, int32_t radius, int32_t X, int32_t *radiuslimit);
/* host only: the number of shells the per-shell sums of a Z x Y x X volume have */
int xh_mono_num_shells(int32_t Z, int32_t Y, int32_t X, int32_t *nshell);
/* every buffer of a Z x Y x X volume (each side 2 .. 1024) */
int xh_mono_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_mono **out);
int xh_mono_destroy(xh_mono *h);
/* ProgMonogenicSignalRes::run (:338-557) with produceSideInfo (:90-166), refiningMask (:203-256) and postProcessingLocalResolutions
 * (:259-335). d_vol: the map, or the first half map with d_vol2 the second (null: single map). d_mask: the --mask volume as int32;
 * d_mask_excl: --maskExcl or null. h_steps (nullable) receives the first max_steps records, *n_steps the number of evaluated
 * frequencies, *stop the reason above. Outputs on the device: d_mean (nullable, written with half maps: meanMap), d_refined int32
 * (refinedMask), d_chimera (monoresResolutionChimera), d_resmap (monoresResolutionMap). Synchronous. */
int xh_mono_run(xh_mono *h, const double *d_vol, const double *d_vol2, const int32_t *d_mask, const int32_t *d_mask_excl, const xh_mono_params *prm,
                xh_mono_step *h_steps, int32_t max_steps, int32_t *n_steps, int32_t *stop, double *d_mean, int32_t *d_refined, double *d_chimera,
                double *d_resmap);
/* after a run: proteinRadiusVolumeAndShellStatistics' radius, findCliffValue's radiuslimit, NVoxelsOriginalMask as the sweep used it;
 * always: the number of shells. Null pointers are skipped */
int xh_mono_info(const xh_mono *h, int32_t *radius, int32_t *radiuslimit, int64_t *nvoxels, int32_t *nshell);
/* test hook: amplitudeMonoSig3D_LPF (:283-415; banded != 0) or monogenicAmplitude_3D_Fourier (:575-661) of the map d_vol, to d_out */
int xh_mono_amplitude(xh_mono *h, const double *d_vol, double freq, double freqH, double freqL, int32_t banded, double *d_out);
/* test hook: realGaussianFilter (data/fourier_filter.cpp :849) of d_vol in place */
int xh_mono_gaussian(xh_mono *h, double *d_vol, double sigma);
/* test hook: the statistics of one (amplitude, mask): d_ampN null is statisticsInOutBinaryMask2 on d_ampS, else statisticsInBinaryMask2;
 * thr95 = sorted noise values [size_t(NN significance)]. An empty noise set is refused */
int xh_mono_statistics(xh_mono *h, const double *d_ampS, const double *d_ampN, const int32_t *d_mask, double significance, xh_mono_stats *out);
/* test hook: element `rank` (from 0) of the sorted values of d_vals [n] whose d_mask is not 0 (null: all), n at most Z Y X */
int xh_mono_select(xh_mono *h, const double *d_vals, const int32_t *d_mask, size_t n, size_t rank, double *out);
/* test hook: setLocalResolutionHalfMaps (halves != 0, :518-539) / setLocalResolutionMap (:548-569) on caller arrays [n], in place */
int xh_mono_assign(xh_mono *h, const double *d_amp, int32_t *d_mask, double *d_res, size_t n, double threshold, double resolution, double resolution_2,
                   int32_t halves);
/* test hook: findCliffValue's per-shell sum, sum2 and N of d_vol about the Xmipp origin, each [xh_mono_num_shells] on the host */
int xh_mono_shell_sums(xh_mono *h, const double *d_vol, double *h_sum, double *h_sum2, double *h_N);
/* for the benchmark: with timing on a run records events around the stages of every frequency (and waits once more per frequency to read
 * them); h_ms[7] = split / filter, the batched inverse line passes, the amplitude row pass, smoothing, statistics, select, assign, summed
 * over the last run's frequencies (both maps with half maps) */
int xh_mono_set_timing(xh_mono *h, int32_t on);
int xh_mono_stage_ms(const xh_mono *h, double *h_ms);

/* ---- xmipp_volume_local_sharpening, LocalDeblur (libraries/reconstruction/volume_local_sharpening.{h,cpp}, ProgLocSharpening) ----
 * Sharpens a map with the local resolution map MonoRes gives: an iteration applies twice the operator L, a bank of narrow band-pass
 * filters (one per resolution, 0.2 A apart) whose outputs are weighted voxel by voxel with exp(-K (res - resVol)^2) and summed. The
 * reference runs fp64 FFTW transforms on CPU threads; here the band filter, the weights and the sum over bands stay on the device and the
 * host reads one small record per iteration. Everything is fp64. The kernels, the reference behaviours kept as written and the refusals
 * are listed at the head of xmipp3_amd/csrc/xh_ldb.hip. Volumes are [Z][Y][X]. */
typedef struct xh_ldb xh_ldb;
/* one iteration of run (:311-398): norm = |op|, porc = lastnorm 100 / norm, subst = porc - lastporc (:345-348), lambda as used by this
 * iteration's update (:360-364, :378), stop: the rule subst < 1 && i > 2 has fired (:350-355) */
typedef struct {
    double norm, porc, subst, lambda;
    int32_t stop, pad_;
} xh_ldb_iter;
/* host only: the bands of localfiltering (:231-244) for a spectrum of zsize planes: res from 2 sampling below max_res in repeated
 * additions of 0.2, a band whose DIGFREQ2FFT_IDX(sampling / res, zsize) equals the last processed one skipped. max_res is the loop's
 * bound, which run sets to the map's maximum + 2 (:298). h_bands [cap][4] receives res, w = sampling / res, wL = sampling / (res - 0.2)
 * and the index of the first cap bands, *n their number. 2 sampling - 0.2 <= 0 is refused */
int xh_ldb_bands(int32_t zsize, double sampling, double max_res, double *h_bands, int32_t cap, int32_t *n);
/* every buffer of a Z x Y x X volume (each side 2 .. 1024), the plans and the spectra of `batch` bands (1 .. 64, rounded up to an even
 * number: two bands share a complex line in the row kernel) */
int xh_ldb_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t batch, xh_ldb **out);
int xh_ldb_destroy(xh_ldb *h);
/* produceSideInfo (:58-130): copies the volume and the resolution map, takes maxRes before the clamp (:132-149), raises resolutions in
 * (0, 2 sampling) to 2 sampling (:115-123), computes desvOutside (:151-179), the band list for maxRes + 2 and lastweight (:263). A map
 * without a voxel at or above 2 sampling is refused. Synchronous */
int xh_ldb_load(xh_ldb *h, const double *d_vol, const double *d_res, double sampling, double K);
/* after a load: maxRes (before the + 2 of run), desvOutside, the number of voxels with resVol < 2 sampling, the number of bands;
 * h_bands [cap][6]: res, w, wL, index, and the band's table of kept lines: kcount (z planes whose y lines are transformed) and jcount
 * (columns kept in every pass). Null pointers are skipped */
int xh_ldb_info(const xh_ldb *h, double *maxRes, double *desvOutside, int64_t *noutside, int32_t *nbands, double *h_bands, int32_t cap);
/* test hook: the clamped resolution map, to d_out */
int xh_ldb_resmap(xh_ldb *h, double *d_out);
/* test hook: localfiltering (:219-283) of the volume d_in, to d_out */
int xh_ldb_localfilter(xh_ldb *h, const double *d_in, double *d_out);
/* run (:285-407) on the loaded volume: at most niter iterations (>= 1), lambda == 1 estimated at the first one (:360-364). h_iters
 * (nullable) receives the first max_iters records, *n_iters the last i, *stopped whether the stop rule ended the loop, *lambda_out the
 * lambda in use at the end (MDL_COST, :400), d_out the sharpened map. Synchronous */
int xh_ldb_run(xh_ldb *h, double lambda, int32_t niter, xh_ldb_iter *h_iters, int32_t max_iters, int32_t *n_iters, int32_t *stopped, double *lambda_out,
               double *d_out);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[5] = forward transforms, split, the y and z line passes, the
 * row pass, finishing, summed since set_timing or the start of the last run */
int xh_ldb_set_timing(xh_ldb *h, int32_t on);
int xh_ldb_stage_ms(const xh_ldb *h, double *h_ms);

/* ---- xmipp_resolution_fso, the Fourier Shell Occupancy (libraries/reconstruction/resolution_fso.{h,cpp}, ProgFSO) ----
 * Two half maps give the global FSC, one directional FSC per direction of a half sphere (each through a Gaussian-weighted cone), the FSO
 * curve with the Bingham isotropy test, the resolution distribution on the projection sphere and, optionally, the 3DFSC. The reference
 * sweeps every Fourier coefficient below Nyquist once per direction on CPU threads; here one pass over the coefficients serves every
 * direction, and the host keeps what is O(directions x shells). The kernels, what is left out and why, and the refusals are listed at the
 * head of xmipp3_amd/csrc/xh_fso.hip. Volumes are [Z][Y][X] doubles; L = X / 2 + 1 shells. */
typedef struct xh_fso xh_fso;
/* host only, replaces the table of generateDirections (:572-898): an icosahedron with one vertex on +z and its upper ring at tilt atan 2,
 * rot 36 + 72 k, `level` (0 .. 5) rounds of edge-midpoint subdivision projected to the sphere, one direction of every antipodal pair,
 * vertices first and then each round's new points, the angles rounded to 4 decimals of a degree. Level 3: 321 directions, level 2: 81.
 * h_rot_tilt_deg [cap][2] receives the first cap, *n their number */
int xh_fso_directions(int32_t level, float *h_rot_tilt_deg, int32_t cap, int32_t *n);
/* host only: degrees to the float radians of :985, then the unit vectors of fscDir_fast :408-410 by sinf / cosf: h_dirs [n][3] */
int xh_fso_unit_vectors(const float *h_rot_tilt_deg, int32_t n, float *h_dirs);
/* host only: incompleteGammaFunction (:510-569). The 41 entries are P(5, i / 2) to 5 significant digits, then to float; the index is
 * round(2 x) clamped to 0 .. 40 */
double xh_fso_incomplete_gamma(double x);
/* host only: the cone's constants as fscDir_fast computes them from --anglecone (run :1344, :419, :425). An angle outside (0, 90) is
 * refused */
int xh_fso_cone(double ang_con_deg, float *cosAngle, float *aux);
/* host only: what run and fscDir_fast do with the sums of every direction, with one thread, the directions in ascending order: the float
 * FSC max(0, num / (sqrt(den1 den2) + 1e-38)) (:468-469) to h_fsc [ndir][L]; the directional resolution, xdim sampling / i at the first
 * i > 2 with FSC <= thrs or -1 (:480-485), to h_resol [ndir]; the FSO curve, shells 0 .. 4 set to 1 (:989-999, :1468-1470), to
 * h_fso [L]; the Bingham statistic of :1426-1464 (the argument of xh_fso_incomplete_gamma) to h_bingham [L]. h_sums [ndir][L][3] */
int xh_fso_decide(const double *h_sums, const float *h_dirs, int32_t ndir, int32_t L, int32_t xdim, double sampling, double thrs, float *h_fsc, double *h_resol,
                  float *h_fso, double *h_bingham);
/* host only: resolutionDistribution (:1194-1261): h_out [360][91], the weighted directional resolution at (rot, tilt) in degrees */
int xh_fso_resolution_distribution(const float *h_dirs, int32_t ndir, const double *h_resol, double ang_con_deg, double *h_out);
/* every buffer of a Z x Y x X box (sides 8 .. 1024; an odd X beside an even Y or Z is refused). seg: the coefficients a workgroup of the
 * cone stage takes, at most 2048; 0 is the default (512) */
int xh_fso_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t seg, xh_fso **out);
int xh_fso_destroy(xh_fso *h);
/* prepareData (:1002-1032) without CenterFFT, the two transforms of run (:1324-1325), defineFrequencies (:111-205) and
 * arrangeFSC_and_fscGlobal (:209-321). d_mask may be null. h_sums [L][3] receives num, den1, den2 of every shell in fp64 (:314-316; the
 * host forms the FSC of :331), h_shell_count [L] (nullable) freqElems, *ncomps (nullable) the number of kept coefficients. Synchronous */
int xh_fso_load(xh_fso *h, const double *d_half1, const double *d_half2, const double *d_mask, double *h_sums, int64_t *h_shell_count, int64_t *ncomps);
/* the shells; after a load: the kept coefficients and the segments of the cone stage; always: seg. Null pointers are skipped */
int xh_fso_info(const xh_fso *h, int64_t *ncomps, int32_t *nshell, int32_t *nseg, int32_t *seg);
/* test hook: the layout of :290-312 on the host, each array [ncomps]: fx, fy, fz, freqidx, arr2indx, real_z1z2, absz1_vec, absz2_vec */
int xh_fso_layout(xh_fso *h, float *h_fx, float *h_fy, float *h_fz, int32_t *h_freqidx, int32_t *h_arr2indx, float *h_real_z1z2, float *h_absz1, float *h_absz2);
/* the sums of fscDir_fast (:428-457) for ndir (1 .. 1024) directions at once. h_dirs [ndir][3]: x_dir, y_dir, z_dir; cosAngle and aux as
 * :419-425 compute them. h_sums [ndir][L][3] receives num, den1, den2 in fp64 (the host forms :468-469), h_count [ndir] the coefficients
 * inside each cone. Two calls give the same bytes. Synchronous */
int xh_fso_directional(xh_fso *h, const float *h_dirs, int32_t ndir, float cosAngle, float aux, double *h_sums, int64_t *h_count);
/* the 3DFSC (:492-507 of every direction in ascending order, :1501-1508, the line fixes :1521-1539) from the directional FSCs
 * h_fsc [ndir][L] (float, as :469 stores them) to d_half [Z][Y][X/2+1] (threeD_FSC.mrc); d_full [Z][Y][X] (nullable) receives
 * createFullFourier (:1297-1306) of it (3dFSC.mrc). Cubic boxes only. The threshold of run enters aniFilter only, which is left out.
 * Synchronous */
int xh_fso_threedfsc(xh_fso *h, const float *h_dirs, int32_t ndir, float cosAngle, float aux, const float *h_fsc, double *d_half, double *d_full);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[5] = the transforms (with the mask), the layout (with the
 * global sums), the cones, the segment reduction, the 3DFSC, summed since set_timing */
int xh_fso_set_timing(xh_fso *h, int32_t on);
int xh_fso_stage_ms(const xh_fso *h, double *h_ms);

/* ---- xmipp_volume_subtraction (libraries/reconstruction/volume_subtraction.{h,cpp}, ProgVolumeSubtraction) ----
 * Adjusts a volume V to a reference V1 by projections onto convex sets (Fourier amplitudes of V1, its value range, the mask, the phases
 * of V, non-negativity, the standard deviation of V1, optionally a low pass) and forms V1 minus the adjusted V inside a mask. The
 * reference runs four to six fp64 FFTW transforms and seven passes per iteration on the CPU; here the volume and its spectrum stay on
 * the device and the host reads two sums per iteration. Everything is fp64. The kernels, the reference behaviours kept as written and
 * the refusals are listed at the head of xmipp3_amd/csrc/xh_vsub.hip. Volumes are [Z][Y][X], spectra [Z][Y][X/2+1]. */
typedef struct xh_vsub xh_vsub;
/* the RMS change of the volume over each step of one runIteration (:376-416), the values computeEnergy (:205-211) forms; filter is 0
 * without cutFreq */
typedef struct {
    double amplitude, minmax, mask, phase, nonneg, scale, filter;
} xh_vsub_energy;
/* host only: the bins of radialAverage (:235) for a box and the largest bin round(w X) its octant writes. --radavg is refused where
 * *maxbin >= *nbins: the reference writes past radial_mean there */
int xh_vsub_radial_bins(int32_t Z, int32_t Y, int32_t X, int32_t *nbins, int32_t *maxbin);
/* the plans and every buffer of a Z x Y x X volume (each side 2 .. 1024) */
int xh_vsub_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_vsub **out);
int xh_vsub_destroy(xh_vsub *h);
/* run :424-427, :432, :435: d_mask (null: ones; copied) times d_V1, max(0, .), its minimum, maximum and stddev, V1FourierMag, and with
 * radavg != 0 V1's radial mean (refused on a box whose bins overflow). Serves any number of adjust calls. Synchronous */
int xh_vsub_set_reference(xh_vsub *h, const double *d_V1, const double *d_mask, int32_t radavg);
/* after set_reference: v1min, v1max, std1, the number of radial bins. Null pointers are skipped */
int xh_vsub_info(const xh_vsub *h, double *v1min, double *v1max, double *std1, int32_t *nbins);
/* test hook: V1FourierMag [Z][Y][X/2+1] to d_out */
int xh_vsub_reference_magnitude(xh_vsub *h, double *d_out);
/* test hook: radialAverage (:223-257) of the magnitude d_mag [Z][Y][X/2+1] to h_mean [nbins]; an empty bin gives NaN as in the reference */
int xh_vsub_radial_mean(xh_vsub *h, const double *d_mag, double *h_mean);
/* test hook: computeRadQuotient (:259-275) of the set reference (with its radial mean) against the volume d_V as it is, to h_quotient [nbins] */
int xh_vsub_quotient(xh_vsub *h, const double *d_V, double *h_quotient);
/* test hook: one runIteration (:362-418) of the volume d_V to d_out, with the phases (and with radavg the quotient) of the volume d_V0;
 * neither is masked or clipped first. Synchronous */
int xh_vsub_iteration(xh_vsub *h, const double *d_V0, const double *d_V, double lambda, int32_t radavg, double cutFreq, double *d_out);
/* run :428-442: mask and max(0, .) of d_V, its phases, the quotient with radavg != 0 (the reference must have been set with it), `iter`
 * (>= 0) times runIteration with lambda in [0, 1] and cutFreq in [0, 0.5] (0: no filter). h_energies (nullable) [iter] receives the
 * energies; d_out has the same bytes with and without them. iter = 0 gives the masked, clipped input. Synchronous */
int xh_vsub_adjust(xh_vsub *h, const double *d_V, int32_t iter, double lambda, int32_t radavg, double cutFreq, xh_vsub_energy *h_energies, double *d_out);
/* FourierFilter LOWPASS RAISED_COSINE, w1 = cutFreq in (0, 0.5], raised_w = 0.02 (createFilter :277-282), of d_in to d_out (may be d_in) */
int xh_vsub_lowpass(xh_vsub *h, const double *d_in, double cutFreq, double *d_out);
/* filterMask (:332-338): FourierFilter LOWPASS REALGAUSSIAN, w1 = sigma >= 0, of d_mask to d_out (may be d_mask) */
int xh_vsub_smooth_mask(xh_vsub *h, const double *d_mask, double sigma, double *d_out);
/* subtraction (:284-306): V1F is d_V1_raw, through xh_vsub_lowpass when cutFreq != 0, and goes to d_V1F (nullable);
 * d_out = V1 (1 - m) + (V1F - min(Vadj, V1F)) m. d_out may be none of the inputs' memory. Synchronous */
int xh_vsub_subtract(xh_vsub *h, const double *d_V1_raw, const double *d_Vadj, const double *d_masksub, double cutFreq, double *d_V1F, double *d_out);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[4] = the transforms, the spectrum steps (amplitude, phase),
 * the real-space steps, the filter (its transforms included), summed over the last adjust */
int xh_vsub_set_timing(xh_vsub *h, int32_t on);
int xh_vsub_stage_ms(const xh_vsub *h, double *h_ms);

/* ---- xmipp_transform_symmetrize (libraries/reconstruction/symmetrize.{h,cpp}, ProgSymmetrize; data/symmetries.cpp:1574-1705) ----
 * Real-space symmetrisation of a volume by a point group or a helix, and of an image stack by a rotation order, with xmippCore's 3-D
 * applyGeometry (LINEAR and BSPLINE3, WRAP and DONT_WRAP) and the 3-D spline prefilter behind it. Everything is fp64; volumes are
 * [Z][Y][X], logical coordinates start at -(dim / 2). xmippCore is not in the reference tree: applyGeometry is the 2-D branch the oracle
 * restates (oracle/xo_bspline.cpp:89-217) with a z axis added; source coordinates are computed directly (x A00 + y A01 + z A02), not by
 * adding A00 along the row. The kernels and the behaviours kept as written are listed at the head of xmipp3_amd/csrc/xh_sym.hip.
 * create: a box of 2 .. 1024 a side; Z = 1 makes a handle for image stacks (symmetrize_images only), Z >= 2 one for volumes. */
typedef struct xh_sym xh_sym;
int xh_sym_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_sym **out);
int xh_sym_destroy(xh_sym *h);
/* the list of a point group: h_R [n][3][3], row-major, the R of SymList::getMatrices without the identity, n = SL.symsNo() (0 .. 1024).
 * Entry i is applied as applyGeometry(.., R.transpose(), IS_NOT_INV, ..) (symmetrize.cpp:150-159): the kernel reads inv(R^T), formed by
 * cofactors. Refused: entries that are not finite, singular matrices, inverses with an entry above 1000 */
int xh_sym_set_matrices(xh_sym *h, const double *h_R, int32_t n);
/* symmetrizeVolume without helix and mask (symmetrize.cpp:117-169): d_out = (V_in + sum_i applyGeometry(degree, V_in, R_i^T, wrap, avg)) times
 * 1.0 / (n + 1.0f) unless sum; avg is the outside mean when !wrap (do_outside_avg = !wrap, :263), else 0. degree 1 or 3 (3: the
 * coefficients are formed first). The sum is kept in a register in the list's order; d_out may not be d_in */
int xh_sym_symmetrize(xh_sym *h, const double *d_in, int32_t degree, int32_t wrap, int32_t sum, double *d_out);
/* symmetrizeImage (symmetrize.cpp:187-214) of a stack d_in [n][Y][X] in one launch, on a Z = 1 handle: I + sum_{i=1}^{order-1}
 * rotate(degree, I, 360.0 / order * i, 'Z', wrap, avg), times 1.0 / order unless sum; avg per image over r^2 >= (min(X, Y) / 2)^2 when !wrap */
int xh_sym_symmetrize_images(xh_sym *h, const double *d_in, int32_t n, int32_t order, int32_t degree, int32_t wrap, int32_t sum, double *d_out);
/* symmetry_Helical (data/symmetries.cpp:1632-1705, mask == nullptr) with interpolatedElement3DHelical (:1577-1630); zHelical in voxels,
 * the angles in radians. dihedral != 0 is symmetrizeVolume's helicalDihedral branch (symmetrize.cpp:172-179): the dihedral copies inside the
 * helix, then rotate(degree, Vrotated, V_out, 180.0, 'X', WRAP) and (V_out + Vrotated) * 0.5. Refused, before any launch: Cn outside 1 .. 99,
 * and parameters for which xh_sym_helical_depth gives -1 */
int xh_sym_helical(xh_sym *h, const double *d_in, double zHelical, double rotHelical, double rotPhaseHelical, int32_t Cn, int32_t dihedral, double heightFraction,
                   int32_t degree, double *d_out);
/* host only: the depth interpolatedElement3DHelical's recursion reaches for the sample points of symmetry_Helical on Z planes: 0 or 1, or -1
 * where it has no bound (zHelical <= 1 voxel, where the reference never terminates; zHelical > Z; heightFraction outside (0, 1]) */
int xh_sym_helical_depth(int32_t Z, double zHelical, double heightFraction, int32_t dihedral, int32_t *depth);
/* hooks for tests and later programs. apply_geometry3d: xmippCore applyGeometry(degree, V2, V1, A, IS_NOT_INV, wrap, outside) for one 3 x 3
 * matrix h_A (row-major, no shifts); an A within 1e-6 of the identity copies (isIdentity). coefficients: produceSplineCoefficients(BSPLINE3)
 * of a volume, x then y then z lines (d_out may be d_in). outside_mean: the mean over r^2 >= (min(dims) / 2)^2 (BinaryCircularMask
 * OUTSIDE_MASK, data/mask.cpp:193-217; the radius by integer division, symmetrize.cpp:133-135), summed in a fixed order. Synchronous */
int xh_sym_apply_geometry3d(xh_sym *h, const double *d_in, const double *h_A, int32_t degree, int32_t wrap, double outside, double *d_out);
int xh_sym_coefficients(xh_sym *h, const double *d_in, double *d_out);
int xh_sym_outside_mean(xh_sym *h, const double *d_in, double *h_mean);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[3] = the coefficients, the outside mean, the symmetry pass
 * (the helix and its dihedral pass included), summed since set_timing */
int xh_sym_set_timing(xh_sym *h, int32_t on);
int xh_sym_stage_ms(const xh_sym *h, double *h_ms);

/* ---- xmipp_volume_align (reconstruction/volume_align_prog.cpp, ProgAlignVolumes; CPU only in the reference): the fitness of many trials
 * per pass over V1 and the mask, fp64. A trial is the reference's 10-vector p: flip, greyScale, greyShift, rot, tilt, psi, scale, z, y, x.
 * Its Vaux = applyTransformation(V2, p, wrap) (:56-97) is never stored: the fit kernel forms every voxel of it in a register and adds what
 * correlationIndex (method 1, COVARIANCE; the fit is minus the index) or rms (method 2, LEAST_SQUARES) need, within the mask (nonzero =
 * inside). The kernels, the one-pass form of the sums and the behaviours kept are listed at the head of xmipp3_amd/csrc/xh_valign.hip.
 * create: a box of 2 .. 1024 a side; capacity (1 .. 2^20) is the most trials of one launch. No output depends on it. */
typedef struct xh_valign xh_valign;
int xh_valign_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t capacity, xh_valign **out);
int xh_valign_destroy(xh_valign *h);
/* uploads V1, V2 [Z][Y][X] and the mask (null: every voxel) from the host, and forms n, mean_x, stddev_x (computeAvgStdev's rule with the
 * integer N / (N - 1)) and S0 = sum (x - mean_x) of V1 within the mask, in raster order. stats: those four, h_stats[4]. Synchronous */
int xh_valign_set_volumes(xh_valign *h, const double *h_V1, const double *h_V2, const int32_t *h_mask);
int xh_valign_stats(const xh_valign *h, double *h_stats);
/* host only: applyTransformation's A = Euler(rot, tilt, psi) with column 2 times flip, times T(x, y, z; z = -z + 1 for flip < 0), times
 * S(scale), h_A [16] row-major; its inverse h_Ainv [16] (cofactor inverse of the 3 x 3 block, -Rinv t); ident: A within 1e-6 of the identity */
int xh_valign_matrix(const double *h_p, double *h_A, double *h_Ainv, int32_t *ident);
/* host only: the trials of the exhaustive search (:363-384) in the reference's order. h_ranges [9][3]: (first, last, step) of grey_scale,
 * grey_shift, rot, tilt, psi, scale, z, y, x; a zero step is 1; the loop variables are doubles advanced by += and tested with <=.
 * h_p [count][10] (null: count only); times (nullable): the progress bar's count (:330-352), which is not the trip count. Refused: more
 * than `limit` trials, and a range whose loop would never end (a negative or vanishing step with first <= last) */
int xh_valign_trials(const double *h_ranges, int32_t consider_mirror, int64_t limit, double *h_p, int64_t *count, int64_t *times);
/* h_fit [m] = fitness(p) of every trial of h_p [m][10], any m, in launches of at most `capacity` trials. search: also the index and fit of
 * the first minimum in trial order (fit < best, :388); h_fit may be null. Synchronous. Refused: a trial with an entry that is not finite
 * or a singular matrix (scale 0) */
int xh_valign_fit(xh_valign *h, const double *h_p, int64_t m, int32_t method, int32_t wrap, double *h_fit);
int xh_valign_search(xh_valign *h, const double *h_p, int64_t m, int32_t method, int32_t wrap, int64_t *best_index, double *best_fit, double *h_fit);
/* d_out [Z][Y][X] = applyTransformation(V2, p, wrap), the grey values included. Synchronous */
int xh_valign_apply(xh_valign *h, const double *h_p, int32_t wrap, double *d_out);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[3] = gather and workgroup sums, finish, choice, summed since
 * set_timing */
int xh_valign_set_timing(xh_valign *h, int32_t on);
int xh_valign_stage_ms(const xh_valign *h, double *h_ms);

/* ---- xmipp_volume_find_symmetry (libraries/reconstruction/volume_find_symmetry.cpp, ProgVolumeFindSymmetry; data/symmetries.cpp:1574-1705
 * for the helix; CPU threads in the reference): the correlation of a volume with its own symmetrised copy for many trials per pass over
 * the volume and the mask, fp64. No symmetrised volume is stored. The kernels, the behaviours kept, the deviations and the refusals are
 * listed at the head of xmipp3_amd/csrc/xh_fsym.hip.
 * create: a box of 2 .. 1024 a side; capacity (1 .. 2^20) is the most trials of one launch. No output depends on it. */
typedef struct xh_fsym xh_fsym;
int xh_fsym_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t capacity, xh_fsym **out);
int xh_fsym_destroy(xh_fsym *h);
/* uploads V [Z][Y][X] and the mask (null: every voxel; nonzero = inside) from the host and forms n, mean, deviation and sum (x - mean) of
 * V within the mask as xh_valign_set_volumes does (:390, :401 take correlationIndex within mask_prm's mask). splines != 0: also the cubic
 * spline coefficients of V (--useSplines, :382-384), through xh_sym_coefficients. stats: those four values, h_stats[4]; clipped != 0:
 * under the mask clipped for the last helical fit. Synchronous */
int xh_fsym_set_volume(xh_fsym *h, const double *h_V, const int32_t *h_mask, int32_t splines);
int xh_fsym_stats(const xh_fsym *h, int32_t clipped, double *h_stats);
/* host only (:373-381): axis = row 2 of Euler_angles2matrix(rot, tilt, 0); h_A [rot_sym - 1][9] = rotation3DMatrix(360.0 / rot_sym * n, axis)
 * for n = 1 .. rot_sym - 1, row-major; h_Ainv their cofactor inverses, which the kernel reads. Either may be null. rotation3DMatrix about
 * an axis is not in the reference tree: the rotation about the unit axis in the sense of rotation3DMatrix(ang, 'Z') */
int xh_fsym_axis_matrices(double rot, double tilt, int32_t rot_sym, double *h_A, double *h_Ainv);
/* host only: the trials of an exhaustive search, two nested loops with double loop variables advanced by += and tested with <= (:221-225
 * rot outer, tilt inner; :293-303 rot outer, z inner). h_p [count][2] = (outer, inner) (null: count only); n_outer, n_inner (nullable):
 * ydim and xdim of the correlation map (:292-303). Refused: more than `limit` trials, and a loop that would never end */
int xh_fsym_grid(double first0, double last0, double step0, double first1, double last1, double step1, int64_t limit, double *h_p, int64_t *count, int64_t *n_outer,
                 int64_t *n_inner);
/* host only (:396-399): gated = 1 where evaluateSymmetry returns 1e38 without any work: zHelical < 0 || zHelical > 0.4 Z, or outside the
 * search box [z0, zF] x [rot0, rotF]. zHelical in voxels */
int xh_fsym_helical_gate(int32_t Z, double zHelical, double rotHelical, double z0, double zF, double rot0, double rotF, int32_t *gated);
/* host only: the depth interpolatedElement3DHelical's recursion (symmetries.cpp:1577-1630) reaches for the sample points of the masked
 * symmetry_Helical this program calls: 0, or 1 for the dihedral copies over an even Z covered entirely with 1 <= zHelical <= Z, or -1
 * where it has no bound or the reference divides by zero (zHelical <= 0, heightFraction outside (0, 1], those dihedral copies with
 * zHelical < 1 or > Z). xh_sym_helical_depth is the bound of the unmasked caller and stays as it is */
int xh_fsym_helical_depth(int32_t Z, double zHelical, double heightFraction, int32_t dihedral, int32_t *depth);
/* --sym rot (:364-391): h_corr [m] = correlationIndex(V, V + sum_n applyGeometry(V, A_n), mask) of every trial (rot, tilt) of
 * h_rot_tilt [m][2], any m, in launches of at most `capacity` trials; LINEAR, or BSPLINE3 when set_volume had splines; DONT_WRAP. search:
 * also the first trial whose correlation is strictly above the running best, which starts at 0 (:167, :188): best_index -1 and best_corr 0
 * where none is, and the caller answers rot = tilt = 0. h_corr may be null in search. Synchronous. Refused: rot_sym outside 2 .. 99,
 * entries that are not finite */
int xh_fsym_axis_fit(xh_fsym *h, const double *h_rot_tilt, int64_t m, int32_t rot_sym, double *h_corr);
int xh_fsym_axis_search(xh_fsym *h, const double *h_rot_tilt, int64_t m, int32_t rot_sym, int64_t *best_index, double *best_corr, double *h_corr);
/* --sym helical | helicalDihedral (:392-417): h_corr [m] = correlationIndex(V, symmetry_Helical(V, z, DEG2RAD(rot), 0, mask, dihedral,
 * heightFraction, Cn), mask) of every trial (rot in degrees, z in voxels: the order of Powell's p, :324-325) of h_rot_z [m][2]. The mask
 * is the one of set_volume zeroed outside [zFirst, zLast] of heightFraction (:280-288), on a copy. h_box (nullable) = z0, zF, rot0, rotF: a
 * trial the gate refuses gets -1e38 on the host without a launch and is never chosen. search: as for the axis. Refused: Cn outside 1 .. 99,
 * entries that are not finite, an ungated trial for which xh_fsym_helical_depth gives -1 */
int xh_fsym_helical_fit(xh_fsym *h, const double *h_rot_z, int64_t m, const double *h_box, int32_t dihedral, double heightFraction, int32_t Cn, double *h_corr);
int xh_fsym_helical_search(xh_fsym *h, const double *h_rot_z, int64_t m, const double *h_box, int32_t dihedral, double heightFraction, int32_t Cn, int64_t *best_index,
                           double *best_corr, double *h_corr);
/* hooks for the tests: the materialised volume_sym of one trial, d_out [Z][Y][X] on the device. axis: every voxel (:378-389); helical:
 * symmetry_Helical's Vout, 0 outside the clipped mask. Synchronous */
int xh_fsym_axis_volume(xh_fsym *h, double rot, double tilt, int32_t rot_sym, double *d_out);
int xh_fsym_helical_volume(xh_fsym *h, double rotHelical, double zHelical, int32_t dihedral, double heightFraction, int32_t Cn, double *d_out);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[3] = gather and workgroup sums, finish, choice, summed since
 * set_timing */
int xh_fsym_set_timing(xh_fsym *h, int32_t on);
int xh_fsym_stage_ms(const xh_fsym *h, double *h_ms);
/* host only, next to xh_halves_circular_mask: BinaryCylinderMask and BinaryTubeMask (data/mask.cpp:471-486, :261-276) with Mask::readParams'
 * modes (:1388-1431): every parameter negative keeps the inside with the absolute values, every one positive the outside; a mix is
 * refused. Kept as written: the cylinder takes |k - z0| <= H / 2, the tube |k| < H (no z0, no half) */
int xh_halves_cylinder_mask(int32_t Z, int32_t Y, int32_t X, double R, double H, double x0, double y0, double z0, int32_t *h_mask);
int xh_halves_tube_mask(int32_t Z, int32_t Y, int32_t X, double R1, double R2, double H, double x0, double y0, double z0, int32_t *h_mask);

/* ---- xmipp_reconstruct_wbp (reconstruction/reconstruct_wbp.cpp, ProgRecWbp; CPU and an MPI farm in the reference): weighted
 * back-projection with the arbitrary-geometry filter, fp64. The handle owns the D^3 volume, the buffers of one batch of `capacity` images,
 * the transform's plans and Tabsinc(0.0001, D) (:538). It reads matrices and direction lists, never angles: the caller forms them, so the
 * device and a restatement read the same doubles. The kernels and the behaviours kept as written are listed at the head of
 * xmipp3_amd/csrc/xh_wbp.hip. create: D of 2 .. 1024, odd sizes included; capacity 1 .. 65535 images of one batch. No output depends on it. */
typedef struct xh_wbp xh_wbp;
int xh_wbp_create(xh_ctx *ctx, int32_t D, int32_t capacity, xh_wbp **out);
int xh_wbp_destroy(xh_wbp *h);
/* a new reconstruction: the volume and count_thr are zero (:526-528). The directions stay */
int xh_wbp_reset(xh_wbp *h);
/* mat_g (:308-359, :231-305): h_g [no_mats][4] = x, y, z, count of every projection direction, symmetry copies included, in the
 * reference's order; threshold: the absolute one, already times totimgs (:304, :358); diameter: 2 * radius, or D (:44, :203-204).
 * Refused: a diameter above D (the reference then reads past its sinc table), entries that are not finite, x, y, z above 1 */
int xh_wbp_set_directions(xh_wbp *h, const double *h_g, int32_t no_mats, double threshold, int32_t diameter);
/* n images through apply2DFilterArbitraryGeometry's loop body (:541-562), in batches of at most `capacity`: h_images [n][D][D] floats,
 * h_rows [n][22] = shiftX, shiftY, flip (0 or not), the weight the image is multiplied by (1 without --weight), the 3 x 3 of
 * Euler_angles2matrix(-rot, tilt, -psi) (:447) and the 3 x 3 inverse of Euler_angles2matrix(rot, -tilt, psi) (:373-374), row-major.
 * prepare (:552-557): A of getTransformationMatrix(A, true) = shifts in column 2, a flip negates A00 and A01; unless A is the identity
 * within 1e-6, selfApplyGeometry(BSPLINE3, ., A, IS_INV, WRAP); times the weight. Then FourierTransform, the filter (:451-487, count_thr
 * grows), InverseFourierTransform and simpleBackprojection into the handle's volume, image after image in list order.
 * h_filtered (nullable): receives the filtered images [n][D][D], what simpleBackprojection read. Synchronous */
int xh_wbp_add(xh_wbp *h, const float *h_images, const double *h_rows, int32_t n, double *h_filtered);
/* :566-579: with nsym > 0 symmetrizeVolume(SL, V, Vaux) at its defaults (symmetrize.h:99-104: BSPLINE3, WRAP, no outside average, no sum)
 * over h_R [nsym][3][3], the R of SL.getMatrices, through xh_sym_symmetrize, then the inner sphere r^2 <= (diameter / 2.)^2;
 * nsym = 0 leaves the volume as it is */
int xh_wbp_finish(xh_wbp *h, const double *h_R, int32_t nsym);
/* the volume [D][D][D] as doubles, to a host or a device pointer; the number of Fourier pixels below the threshold so far (:480) */
int xh_wbp_volume(xh_wbp *h, double *out);
int xh_wbp_count_thr(xh_wbp *h, int64_t *count);
/* hooks for the tests. weights: the filter's weight at every cell for one image's row, h_weights [D][D] in the transform's uncentred
 * layout (cell (iy, jx) holds logical i = iy or iy - D); neither the volume nor count_thr changes. table: the sinc table, *n its
 * length, h_table nullable. tile: the directions of one LDS tile of the filter */
int xh_wbp_weights(xh_wbp *h, const double *h_row, double *h_weights);
int xh_wbp_table(const xh_wbp *h, double *h_table, int64_t *n);
int xh_wbp_tile(void);
/* host only, what the program forms before any device is opened. image_matrices: h_dir[3] = row 2 of Euler_angles2matrix(rot, -tilt, psi)
 * (:327-330), h_filter[9] = Euler_angles2matrix(-rot, tilt, -psi) (:447), h_back[9] = the cofactor inverse of Euler_angles2matrix(rot,
 * -tilt, psi) (:373-374). even_distribution: make_even_distribution(rotList, tiltList, sampling, SL, true) of reconstruction/directions.cpp
 * :133-183 for an empty SL (directions_are_unique with Euler_another_set = (rot + 180, -tilt)); *n the count, h_rot / h_tilt nullable.
 * nearest_direction: find_nearest_direction (:194-237) for an empty SL, -1 for an empty list */
int xh_wbp_image_matrices(double rot, double tilt, double psi, double *h_dir, double *h_filter, double *h_back);
int xh_wbp_even_distribution(double sampling, double *h_rot, double *h_tilt, int32_t capacity, int32_t *n);
int xh_wbp_nearest_direction(double rot, double tilt, const double *h_rot, const double *h_tilt, int32_t n, int32_t *index);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[5] = prepare, both transforms, the filter, the
 * back-projection, finish, summed since set_timing */
int xh_wbp_set_timing(xh_wbp *h, int32_t on);
int xh_wbp_stage_ms(const xh_wbp *h, double *h_ms);

/* ---- xmipp_ctf_estimate_from_micrograph --dont_estimate_ctf and xmipp_psd_estimate: the PSD of a micrograph by periodogram averaging
 * (reconstruction/ctf_estimate_from_micrograph.cpp run() :289-584 in doubles, reconstruction/psd_estimator.cpp estimatePSD :74-148 in
 * floats). The handle holds one micrograph [Y][X] in float32, the two separable taper vectors of constructPieceSmoother (:143-189), a
 * half-spectrum intermediate of `capacity` pieces and the running sums. The kernels are listed at the head of xmipp3_amd/csrc/xh_psd.hip.
 * create: piece sides py, px of 2 .. 1024, odd ones included; the double path (is_double) takes square pieces; capacity 1 .. 65535 pieces
 * of one batch. No output depends on the capacity. */
typedef struct xh_psd xh_psd;
int xh_psd_create(xh_ctx *ctx, int32_t Y, int32_t X, int32_t py, int32_t px, int32_t capacity, int32_t is_double, xh_psd **out);
int xh_psd_destroy(xh_psd *h);
/* the micrograph [Y][X] from a host (pageable or page-locked) or a device pointer: M_in.read (:373). The running sums stay */
int xh_psd_load(xh_psd *h, const float *micrograph);
/* the pieces at h_corners [n][2] = (top row, left column), in list order, `capacity` at a time (:416-463; psd_estimator.cpp:100-117).
 * flags: 1 statisticsAdjust(0, 1) (:422; psd_estimator.cpp:105), 2 normalize_ramp (:423, data/normalize.cpp:333-425; double only).
 * h_stack null: every piece's PSD is added to the running sums (in double its square too), in list order whatever the capacity.
 * h_stack [n][py][px] of the element type: receives each piece's own complete PSD and the sums stay (the regions and particles modes,
 * :497-508). Refused: a corner whose piece leaves the micrograph. Synchronous */
int xh_psd_add(xh_psd *h, const int32_t *h_corners, int32_t n, int32_t flags, void *h_stack);
/* [py][px] of the element type, mirrored by half2whole (psd_estimator.h:52-73). double: avg = sum * (1 / n) and
 * std = sqrt(max(0, sum2 * (1 / n) - avg^2)) (:572-583). float: h_avg receives the SUM of the magnitudes, which is what
 * psd_estimator.cpp:115-121 keeps, h_std zeros. h_std and n nullable; *n the pieces added since reset */
int xh_psd_result(xh_psd *h, void *h_avg, void *h_std, int64_t *n);
/* zero sums, zero pieces; the micrograph stays */
int xh_psd_reset(xh_psd *h);
/* test hooks: the taper (1 * maskY[i]) * maskX[j] [py][px] as the kernels form it; the prepared pieces [n][py][px] before the transform */
int xh_psd_smoother(xh_psd *h, void *h_out);
int xh_psd_piece(xh_psd *h, const int32_t *h_corners, int32_t n, int32_t flags, void *h_out);
/* the columns of the half spectrum one workgroup of the column pass owns */
int xh_psd_strip(void);
/* for the benchmark: with timing on every stage is followed by a wait; h_ms[4] = statistics, rows, columns + accumulate, finish */
int xh_psd_set_timing(xh_psd *h, int32_t on);
int xh_psd_stage_ms(const xh_psd *h, double *h_ms);
/* host only. pieces: the corner list of run() (:310-327, :371-414) with the skip rule and the clamp to the far edge. mode 0 micrograph
 * (step (int)((1 - overlap) pieceDim)), 1 regions (step pieceDim; fewer than 2 skipBorders + 1 divisions is the reference's own error),
 * 2 particles (h_pos [npos][2] = x, y of the centres; a coordinate below pieceDim / 2 is refused: the reference's unsigned subtraction
 * wraps there). h_corners [capacity][2], h_slots [capacity] (the reference's 1-based N of each kept piece), both nullable: *n alone.
 * Refused: a list with no piece, where the reference divides by zero. *div_number (nullable): div_Number.
 * patches: getPatchesLocation (psd_estimator.cpp:35-71), its asserts as refusals */
int xh_psd_pieces(int32_t Y, int32_t X, int32_t pieceDim, double overlap, int32_t skipBorders, int32_t mode, const int64_t *h_pos, int32_t npos,
                  int32_t *h_corners, int32_t *h_slots, int32_t capacity, int32_t *n, int32_t *div_number);
int xh_psd_patches(int32_t Y, int32_t X, int32_t py, int32_t px, int32_t borderX, int32_t borderY, float overlap, int32_t *h_corners, int32_t capacity,
                   int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* XMIPP_HIP_H */
