/*
 * brainfm_hip.h -- C ABI of libbrainfm_hip.so (gfx950 / MI355X).
 *
 * The reference (jhuldr/BrainFM) is pure Python on stock torch ops: it has no
 * FFI of its own.  This header is therefore the boundary a maintainer would
 * bind with ctypes; every entry point cites the reference
 * call chain it replaces.  Conventions:
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - activations are fp32, channels-last-3D: index = ((z*H + y)*W + x)*C + c
 *     (the reference's NCDHW tensors viewed with torch.channels_last_3d strides);
 *   - no allocation, no global state, no host synchronisation inside a call:
 *     the caller owns every buffer (including workspaces) and the stream;
 *   - return value: 0 = launched, <0 = rejected before launch (BFM_E_*).
 */
#ifndef BRAINFM_HIP_H
#define BRAINFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bfm_stream_t; /* hipStream_t */

#define BFM_OK 0
#define BFM_E_ARG (-1)      /* null pointer / non-positive size */
#define BFM_E_SHAPE (-2)    /* shape not supported by this kernel family */
#define BFM_E_WORKSPACE (-3)/* workspace too small */
#define BFM_E_LAUNCH (-4)   /* hipGetLastError() != hipSuccess after launch */

/* Nearest-neighbour upsampling source (F.interpolate(mode='nearest'),
 * Trainer/models/unet3d/buildingblocks.py:361-363): low-res dims and per-axis
 * index maps map?[dst] = min(floor(dst*in/out), in-1) plus replication counts
 * rep?[src] = #{dst : map[dst]==src}.  All six arrays live on the device. */
typedef struct {
    int d, h, w;
    const int32_t* mapD; const int32_t* mapH; const int32_t* mapW; /* len D,H,W of the hi-res grid */
    const int32_t* repD; const int32_t* repH; const int32_t* repW; /* len d,h,w */
} bfm_upsample_t;

/* Library / build info: "brainfm_hip <version> gfx950". */
const char* bfm_version(void);

/* ---------------------------------------------------------------- GroupNorm
 * nn.GroupNorm(G, C, eps) statistics (buildingblocks.py:48-60) over the
 * virtual concatenation cat((A, nearest_up(B)), channel) of Decoder._joining
 * (buildingblocks.py:265-276).  CB==0 / B==NULL for a plain tensor.
 * Outputs the folded affine y = x*scale[c] + shift[c]
 * (scale = gamma*rstd, shift = beta - mean*scale) and, per group, the largest
 * |y| the folded affine can produce (bound[g]) which the MFMA convolution
 * uses to pick a power-of-two operand scale.
 * workspace: bfm_gn_stats_workspace(...) bytes.
 *
 * Arithmetic: sums and sums of squares of the tensor pass are fp64 from the first addition (one pass, var = E[x^2] -
 * mean^2 clamped at 0), so var is good to about (N + 4) 2^-53 E[x^2] for N values per group whatever the summation
 * order: 4e-8 of var on a field whose mean is 10^3 standard deviations.  mean / rstd / scale / shift are the fp32
 * roundings of the fp64 results; bound[g] is, in fp32, max over the group's channels of
 * max(|fmaf(min_c, scale, shift)|, |fmaf(max_c, scale, shift)|), folded with fmaxf from 0.
 * Non-finite input: an Inf or a NaN anywhere in a group makes that group's mean or var non-finite, hence every scale
 * and shift of the group NaN (nn.GroupNorm gives NaN there too); other groups are untouched.  fmaxf drops NaN, so such
 * a group's bound[g] is 0, not NaN: a consumer must not read bound[g] == 0 as "this group is all zero".
 * (tests/test_gpu_gn_pool.py pins both.) */
size_t bfm_gn_stats_workspace(int CA, int CB, int D, int H, int W, const bfm_upsample_t* up);
/* Host arithmetic only, no launch: the pass bfm_gn_stats makes over one source of C channels and nvox voxels whose base
 * pointer is (aligned != 0) or is not 16-byte aligned.  route: float4 lanes need C % 4 == 0 and the alignment, else
 * scalar lanes; with CV = C / 4 (float4) or C (scalar) columns, CV <= 256 keeps rows_in_flight = 256 / CV voxel rows
 * per workgroup (threads beyond rows_in_flight * CV idle), CV > 256 is the wide form: a thread per column, laps of
 * 256 columns, rows_in_flight = 0.  nblocks workgroups of vox_per_block consecutive voxels each (the last one shorter):
 * nblocks = min(clamp(32768 / C, 8, 2048), ceil(nvox / 16)), then evened out.  Any output pointer may be NULL. */
#define BFM_GN_ROUTE_ROWS_VEC4 0
#define BFM_GN_ROUTE_ROWS_SCALAR 1
#define BFM_GN_ROUTE_WIDE_VEC4 2
#define BFM_GN_ROUTE_WIDE_SCALAR 3
int bfm_gn_stats_plan(int C, int64_t nvox, int aligned, int* route, int* nblocks, int64_t* vox_per_block,
                      int* rows_in_flight);
int bfm_gn_stats(const float* A, int CA, const float* B, int CB, int D, int H, int W,
                 const bfm_upsample_t* up, const float* gamma, const float* beta, int G, float eps,
                 float* scale, float* shift, float* bound, void* workspace, size_t workspace_bytes,
                 bfm_stream_t stream);
/* same, also returning the per-group mean and 1/sqrt(var+eps) (G floats each) that the backward pass needs */
int bfm_gn_stats_train(const float* A, int CA, const float* B, int CB, int D, int H, int W, const bfm_upsample_t* up,
                       const float* gamma, const float* beta, int G, float eps, float* scale, float* shift,
                       float* bound, float* mean_out, float* rstd_out, void* workspace, size_t workspace_bytes,
                       bfm_stream_t stream);

/* ------------------------------------------------------ 3x3x3 convolution
 * SingleConv 'gcl' minus the statistics: y = LeakyReLU_slope( conv3d_p1(
 *   x*scale + shift ) )  with x = cat((A, nearest_up(B))).  Zero padding is
 * applied AFTER the affine, as nn.Conv3d pads GroupNorm's output
 * (buildingblocks.py:31-60).  Weights: see bfm_pack_conv_weights_*.
 *
 * _direct: exact fp32 FMA, any Cin/Cout (stem Cin=1, odd widths).
 *   wpacked layout [27][Cin][Cout] fp32.
 * _mfma: implicit GEMM on v_mfma_f32_32x32x16_f16.  Requires CA%16==0,
 *   CB%16==0, Cout%64==0.  passes=3 splits both operands into f16 hi+lo
 *   (hi*hi + hi*lo + lo*hi, fp32 accumulate: ~2^-22 relative product error);
 *   passes=1 uses hi only (fast mode, ~2^-11).  `bound` = G per-group bounds
 *   from bfm_gn_stats (operand scale is derived from them on the device).
 *   splitk>1 needs workspace of splitk*nvox*Cout*4 bytes. */
int bfm_pack_conv_weights_direct(const float* w_oidhw, int Cin, int Cout, float* wpacked, bfm_stream_t stream);
size_t bfm_pack_conv_weights_mfma_bytes(int Cin, int Cout);
/* wmax_abs_host = max|w| (host scalar); returns the power-of-two weight scale exponent in *wexp_host */
int bfm_pack_conv_weights_mfma(const float* w_oidhw, int Cin, int Cout, float wmax_abs_host, void* wpacked,
                               int* wexp_host, bfm_stream_t stream);

/* Layout for the v_mfma_f32_16x16x32_f16 kernel variant (plan cfg[6] == 2): K = 32 is a pair of taps x 16
 * channels.  A layer planned with cfg[6] == 2 must be given weights packed by this function; cfg[6] in {0,1}
 * takes bfm_pack_conv_weights_mfma's layout. */
size_t bfm_pack_conv_weights_mfma16_bytes(int Cin, int Cout);
int bfm_pack_conv_weights_mfma16(const float* w_oidhw, int Cin, int Cout, float wmax_abs_host, void* wpacked,
                                 int* wexp_host, bfm_stream_t stream);

int bfm_conv3x3x3_direct(const float* A, int CA, const float* B, int CB, int D, int H, int W,
                         const bfm_upsample_t* up, const float* scale, const float* shift,
                         const float* wpacked, int Cout, float slope, float* out, bfm_stream_t stream);

/* Cin == 1 stem (enc0.1) as a K = 32 (27 taps + padding) GEMM on the matrix core, same split-fp16 numerics as
 * _mfma; Cout in {32, 64}; weights in the _direct layout [27][Cout]; bound = the single GroupNorm bound
 * (bfm_conv3x3x3_stem_ex). */

/* Winograd F(2,3)-along-x variant of the single-source 3x3x3 conv (SingleConv 'gcl', buildingblocks.py:31-60):
 * 4 transformed positions x 9 (kd,kh) taps for every pair of x-neighbouring outputs = 1.5x fewer matrix-core FLOPs
 * than bfm_conv3x3x3_mfma, same split-fp16 products, fp32 transforms (fp32-grade, not bit-identical to _mfma).
 * No second source, no split-K; `accumulate` as cfg[7] bit 0 of _mfma.  Weights packed by _pack_conv_weights_wino. */
size_t bfm_pack_conv_weights_wino_bytes(int Cin, int Cout, int passes);
int bfm_pack_conv_weights_wino(const float* w_oidhw, int Cin, int Cout, float wmax_abs_host, int passes, void* wpacked,
                               int* wexp_host, bfm_stream_t stream);
int bfm_conv3x3x3_wino_rows(int D, int H, int W, int passes);   /* moment rows of the 4-wave kernel (0: cannot run) */
int bfm_conv3x3x3_wino_ex(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                          const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                          int flags, float* out, void* moment_rows /*or NULL;
 4-wave kernel only*/, bfm_stream_t stream);

/* The last convolution of a tile inside the tile loop (scripts/demo_test.py:88-100 keeps `v * (tile_input != 0)` of every
 * output): a box of output voxels whose tile-input voxels are all zero feeds nothing that survives the mask, so it is not
 * computed (`out` keeps whatever it held there).  mask_image = the tile's input (D,H,W).  The 4-wave kernel, no moment rows. */
/* Boxes that multiply the same operands as other boxes.  Where the network's one-channel input image is bitwise constant
 * (the zero background of a skull-stripped head, utils/test_utils.py:235-284 min-max normalises it to exact zeros) the
 * activations of the first layers depend on the distances to the tile's faces only (zero padding): stem output where the
 * image is constant within 1 voxel, encoders.0 second conv within 2, and so on.  bfm_uniform_boxes flags the boxes of the
 * 4-wave Winograd kernel's grid over which `image` is constant within `radius` voxels (clipped to the volume) with
 * 1 + class, class = 9 cz + 3 cy + cx, c = 0 / 1 / 2 for the first / a middle / the last box along the axis: all boxes of
 * a class see the faces the same way (a box side must be >= radius: BFM_E_SHAPE otherwise).  flags:
 * bfm_uniform_boxes_bytes() bytes, 4-byte aligned: one byte per box, then the first box of each of the 27 classes.
 * bfm_conv3x3x3_wino_uniform is bfm_conv3x3x3_wino_ex that computes the unflagged boxes and the first flagged box of each
 * class in full, and gives every other flagged box its class's accumulators (the bits its own main loop would produce: same
 * operands, same order) before the normal epilogue -- no staging, weights or matrix products there.  Without accumulation
 * (flags bit 0 clear) those boxes' outputs, pooled outputs and moment rows are the first box's, and are copied from it.
 * scratch: bfm_conv3x3x3_wino_uniform_scratch(Cout) bytes, 16-byte aligned (written by accumulating calls only).  The
 * caller passes radius = (number of 3x3x3
 * convolutions between the image and this layer's OUTPUT): 2 for encoders.0's second conv, 3 for the skip half of the last
 * decoder's first conv.
 * Stores by need (flags bit 1 of the _uniform entry points).  The flag buffer ends with a table need[box] = 1 for a flagged
 * box that is not its class's first and has, among its up to 26 neighbours in the grid, a box that is computed in full
 * (unflagged, or a class's first) -- a computed box stages its input with a one-voxel halo, so when the only reader of
 * `out` is a _uniform launch on the SAME flag buffer, the other class mates' voxels are never read.  With bit 1 set,
 * bfm_conv3x3x3_wino_uniform[_pool] without accumulation and bfm_conv3x3x3_wino4_uniform with it leave `out` untouched in
 * those boxes (the other forms store every box as without the bit); every box that is stored holds the same bits, and the
 * moment rows, the pooled tensor and its rows are complete either way.  The caller answers for the reader. */
size_t bfm_uniform_boxes_bytes(int D, int H, int W, int passes);
int bfm_uniform_boxes(const float* image, int D, int H, int W, int radius, int passes, unsigned char* flags,
                      bfm_stream_t stream);
/* the same for a layer `level` MaxPool3d(2) steps down: the box grid is that of the (D >> level, ...) tensor, a box covers
 * image voxels [z0 << level, (z0 + TD) << level), and radius is in IMAGE voxels: 2 * 2^0 for the two level-0 convolutions
 * plus 2^level per convolution at the layer's own level up to its output (4, 6, 8 for the three level-1 layers that read the
 * first activations: encoders.1 conv 1 / conv 2 and the skip half of the second-to-last decoder's conv 1).  flags:
 * bfm_uniform_boxes_bytes(D >> level, H >> level, W >> level, passes) bytes. */
int bfm_uniform_boxes_level(const float* image, int D, int H, int W, int level, int radius, int passes, unsigned char* flags,
                            bfm_stream_t stream);
/* bfm_uniform_boxes_level for several levels of one image in one launch (a tile's encoder pools its first activations once,
 * Encoder.forward, buildingblocks.py:185-186, so levels 0 and 1 both have layers that read them): flags[i] receives, byte
 * for byte, what bfm_uniform_boxes_level(levels[i], radii[i]) writes.  1 <= nlevels <= 4; levels, radii and flags are host
 * arrays.  ticket: one int on the device, 4-byte aligned, zero before the first call and left zero by every call; calls
 * that may run concurrently take different tickets.  BFM_E_SHAPE when any level has no box grid or a box side shorter than
 * its radius (nothing launched: ask level by level then). */
int bfm_uniform_boxes_levels(const float* image, int D, int H, int W, int nlevels, const int* levels, const int* radii,
                             int passes, unsigned char* const* flags, int* ticket, bfm_stream_t stream);
/* completes an `out` (D,H,W,Cout) that a non-accumulating bfm_conv3x3x3_wino_uniform[_pool] launch stored by need: every
 * class mate's box becomes the copy of its class's first box that the launch without bit 1 makes */
int bfm_uniform_fill(float* out, int D, int H, int W, int Cout, int passes, const unsigned char* uniform_flags,
                     bfm_stream_t stream);
size_t bfm_conv3x3x3_wino_uniform_scratch(int Cout);
int bfm_conv3x3x3_wino_uniform(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                               const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                               int flags, float* out, void* moment_rows, const unsigned char* uniform_flags, void* scratch,
                               bfm_stream_t stream);
/* SingleConv followed by nn.MaxPool3d(2) (Encoder.forward, buildingblocks.py:185-186, 211-214: the pooling of the next
 * encoder level reads this layer's output) in one pass: out and moment_rows as bfm_conv3x3x3_wino_ex / _wino_uniform write
 * them (the skip connection keeps the full-resolution tensor), pooled (D/2,H/2,W/2,Cout) = the bits of bfm_maxpool2(out), and
 * pooled_rows (or NULL) = that tensor's moment rows, [bfm_conv3x3x3_wino_rows()][Cout].  The 2 x 2 x 2 windows must be whole
 * inside one box of the kernel: bfm_conv3x3x3_wino_pool_ok() says whether a (D,H,W) tensor qualifies (its box is 8 x 8 x 4
 * and tiles it exactly -- the 80- and 160-voxel tiles of the reference tiling at levels 0 and 1 do); BFM_E_SHAPE otherwise,
 * nothing launched: pool with bfm_maxpool2_ex then. */
int bfm_conv3x3x3_wino_pool_ok(int D, int H, int W, int passes);
int bfm_conv3x3x3_wino_pool(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                            const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                            int flags, float* out, void* moment_rows, float* pooled, void* pooled_rows /*or NULL*/,
                            bfm_stream_t stream);
int bfm_conv3x3x3_wino_uniform_pool(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                                    const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope,
                                    int passes, int flags, float* out, void* moment_rows,
                                    const unsigned char* uniform_flags, void* scratch, float* pooled,
                                    void* pooled_rows /*or NULL*/, bfm_stream_t stream);
int bfm_conv3x3x3_wino_box(int D, int H, int W, int passes, int* box /* [3]: the (d,h,w) box of output voxels per workgroup */);
/* workspace: bfm_conv3x3x3_wino_masked_workspace(D, H, W, passes) bytes (4-byte aligned) for the per-box activity, the
 * number of boxes that hold input and their list, built on the device ahead of the persistent launch that walks it. */
size_t bfm_conv3x3x3_wino_masked_workspace(int D, int H, int W, int passes);
int bfm_conv3x3x3_wino_masked(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                              const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                              int flags, float* out, const float* mask_image, void* workspace, size_t workspace_bytes,
                              bfm_stream_t stream);

/* Output-moment rows.  A producer (conv3x3x3_mfma_ex / conv3x3x3_stem_ex) can write, next to its output, one row
 * per tile of per-channel {sum, sumsq} (fp64) and {min, max} (fp32) of the values it stored: buffer of
 * bfm_moment_rows_bytes(nrows, Cout) bytes laid out sum[nrows][C] | sumsq[nrows][C] | min[nrows][C] | max[nrows][C].
 * The consumer's GroupNorm (nn.GroupNorm in the next SingleConv, buildingblocks.py:48-60) then reduces the rows with
 * bfm_gn_stats_rows instead of re-reading the activation.  Deterministic: fixed reduction order, no atomics.
 * bfm_conv3x3x3_mfma_rows returns 0 when the plan cannot emit rows (split-K or the persistent variant). */
size_t bfm_moment_rows_bytes(int nrows, int C);
int bfm_conv3x3x3_mfma_rows(int Cin, int Cout, int D, int H, int W, const int* cfg);
int bfm_conv3x3x3_mfma_ex(const float* A, int CA, const float* B, int CB, int D, int H, int W,
                          const bfm_upsample_t* up, const float* scale, const float* shift, const float* bound,
                          int G, const void* wpacked, int wexp, int Cout, float slope, int passes, const int* cfg,
                          float* out, void* workspace, size_t workspace_bytes, void* moment_rows /*or NULL*/,
                          bfm_stream_t stream);
/* A batch of S same-shape samples (the tiles of one volume that share a shape) through ONE launch: A [S][D,H,W,CA],
 * B [S][d,h,w,CB], out [S][D,H,W,Cout], scale / shift [S][CA+CB], bound [S][G] -- GroupNorm statistics stay per
 * sample (buildingblocks.py:48-60).  Every workgroup does what it does in the one-sample launch (same box, K order and
 * split-K), so the result is bit-identical to S calls of bfm_conv3x3x3_mfma_ex; what changes is that the S workgroups
 * needing the same packed-weight fragments run side by side and read them from HBM once (the deep levels are bound by
 * their 1 GB of weights per tile).  Plan variants 0 and 2 only; moment_rows: [S * rows][Cout].
 * affine_stride: floats between two samples' scale / shift rows (0 = CA + CB; wider when the caller hands a column
 * window of a wider [S][C] table, e.g. the skip half of a decoder concat). */
size_t bfm_conv3x3x3_mfma_batch_workspace(int Cin, int Cout, int S, int D, int H, int W, int splitk);
int bfm_conv3x3x3_mfma_batch(const float* A, int CA, const float* B, int CB, int S, int D, int H, int W,
                             const bfm_upsample_t* up, const float* scale, const float* shift, const float* bound, int G,
                             const void* wpacked, int wexp, int Cout, float slope, int passes, const int* cfg, float* out,
                             void* workspace, size_t workspace_bytes, void* moment_rows, int affine_stride,
                             bfm_stream_t stream);
/* GroupNorm statistics of such a batch: per sample exactly bfm_gn_stats / bfm_gn_stats_rows (same block split, same
 * summation order), outputs [S][C] / [S][G]. */
size_t bfm_gn_stats_batch_workspace(int CA, int CB, int S, int D, int H, int W, const bfm_upsample_t* up);
int bfm_gn_stats_batch(const float* A, int CA, const float* B, int CB, int S, int D, int H, int W,
                       const bfm_upsample_t* up, const float* gamma, const float* beta, int G, float eps, float* scale,
                       float* shift, float* bound, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_gn_stats_rows_batch(const void* rowsA, int nrowsA_per_sample, int CA, const void* rowsB, int nrowsB_per_sample,
                            int CB, double weightB, int64_t nvox, int S, const float* gamma, const float* beta, int G,
                            float eps, float* scale, float* shift, float* bound, bfm_stream_t stream);

/* nn.MaxPool3d(2) (buildingblocks.py:185-186): window 2, stride 2, floor (the last plane of an odd extent is never
 * read), NaN from any corner kept.  float4 lanes when C % 4 == 0 and both pointers are 16-byte aligned, scalar lanes
 * otherwise; D, H, W >= 2 (BFM_E_ARG).  Moment rows of the pooled tensor: bfm_maxpool2_rows() rows, one per workgroup,
 * 0 (none: asking for them is BFM_E_SHAPE) unless C % 4 == 0, C / 4 <= 256 and 256 % (C / 4) == 0, and only with
 * aligned pointers.  A row's sums are fp32 inside a thread (fs += m, fq = fmaf(m, m, fq) over the
 * ceil(items / (rows * 256)) items of its grid-stride loop, items = d*h*w*C/4), widened to fp64 and folded in thread
 * order; min and max are exact.  See bfm_gn_stats_rows for what that costs on an offset field. */
int bfm_maxpool2_rows(int C, int D, int H, int W);
int bfm_maxpool2_ex(const float* in, int C, int D, int H, int W, float* out, void* moment_rows /*or NULL*/,
                    bfm_stream_t stream);
/* nn.MaxPool3d(2) (buildingblocks.py:185-186) of S same-shape samples in one launch (the batched levels); moment rows
 * [S * bfm_maxpool2_batch_rows()][C] (at most 128 per sample: bfm_gn_stats_rows_batch reads them directly).  A sample's
 * output and rows do not depend on S.  C % 4 == 0. */
int bfm_maxpool2_batch_rows(int C, int D, int H, int W);
int bfm_maxpool2_batch(const float* in, int C, int S, int D, int H, int W, float* out, void* moment_rows /*or NULL*/,
                       bfm_stream_t stream);
int bfm_conv3x3x3_stem_rows(int D, int H, int W);
int bfm_conv3x3x3_stem_ex(const float* A, int D, int H, int W, const float* scale, const float* shift,
                          const float* bound, const float* wpacked_direct, int Cout, float slope, float* out,
                          void* moment_rows /*or NULL*/, bfm_stream_t stream);
/* The stem of a conditioned network, Cin in {2, 3, 4} (build_conditioned_model / build_inpaint_model,
 * Trainer/models/__init__.py:423-463: backbone.py:21-26 with num_cond; the first SingleConv is GroupNorm(1, Cin) +
 * Conv3d(Cin, Cout, 3), buildingblocks.py:31-60): K = 27 * Cin (+ zero columns to a multiple of 16) on the matrix core,
 * A channels-last [D][H][W][Cin] (aligned to Cin floats for Cin 2 and 4), scale / shift per channel, one bound,
 * weights in the _direct layout [27][Cin][Cout], Cout in {32, 64}, D*H*W*Cin < 2^31 (BFM_E_SHAPE otherwise).
 * Moment rows: bfm_conv3x3x3_stem_rows(D, H, W). */
int bfm_conv3x3x3_stem_mc_ex(const float* A, int Cin, int D, int H, int W, const float* scale, const float* shift,
                             const float* bound, const float* wpacked_direct, int Cout, float slope, float* out,
                             void* moment_rows /*or NULL*/, bfm_stream_t stream);
/* GroupNorm scale/shift/bound from moment rows.  Source A: rowsA [nrowsA][CA]; optional source B (the low-res half of
 * a decoder concat, every voxel replicated weightB times by the nearest upsample: 8 for an exact 2x): rowsB.
 * nvox = voxels per channel of the normalised tensor (D*H*W of the full-res grid). */
size_t bfm_gn_stats_rows_workspace(int nrowsA, int CA, int nrowsB, int CB);
/* ticket: NULL, or BFM_GN_TICKETS int32 in device memory that are ZERO before the first call and are left zero by every
 * call (a buffer of its own: nothing else may write it; one per stream that may run these calls concurrently).  With
 * tickets, a table of more than 128 rows and G <= BFM_GN_TICKETS the whole thing is ONE launch: workgroup (group, row
 * slice) folds its slice for the group's channels, the last workgroup of a group to finish runs the group's finalize.
 * Without, it is up to three launches (a fold per large table, then the finalize).  Both forms are deterministic (fixed
 * summation orders); they differ from each other in the last bits of the fp64 sums.
 *
 * Conditioning: the rows are folded in fp64, but every producer (bfm_maxpool2_ex, the conv epilogues) squares and sums
 * in fp32 inside a thread before it widens, so the statistics carry the producer's fp32 error: for a thread that
 * visits j values, |dS| <= (j-1) 2^-24 sum|x| and |dQ| <= j 2^-24 sum x^2.  The error of var relative to var grows
 * with (mean / std)^2: harmless on centred activations, about j 2^-24 (mean/std)^2 on an offset field, where the
 * tensor pass of bfm_gn_stats stays at 2^-53.  Measured on a pooled 10^3 x 64 field with mean/std = 52 (one item per
 * thread, so only the squares round): rstd off by 6.8e-7 from the rows, 3.6e-8 from the tensor pass, 1.0e-7 from
 * torch's fp32 group_norm; on a centred field (mean/std = 2.7) all three are at 3e-8 .. 9e-8
 * (tests/test_gpu_gn_pool.py, test_chain_pool_rows_against_tensor_pass).  Non-finite rows and bound[g]: as bfm_gn_stats. */
#define BFM_GN_TICKETS 16
/* Host arithmetic only: which of the forms above a call takes.  DIRECT: no table has more than 128 rows, the finalize
 * reads them as they lie (one launch, tickets ignored).  ONE_LAUNCH: a table has more than 128 rows, has_ticket,
 * G <= BFM_GN_TICKETS and 16 * (CA + CB) * 24 bytes fit the fold workspace (128 * C * 24 bytes, rounded up to 256, per
 * table of more than 128 rows).  FOLD otherwise.  Negative: the BFM_E_* the call itself would return for these sizes. */
#define BFM_GN_ROWS_DIRECT 0
#define BFM_GN_ROWS_FOLD 1
#define BFM_GN_ROWS_ONE_LAUNCH 2
int bfm_gn_stats_rows_route(int nrowsA, int CA, int nrowsB, int CB, int G, int has_ticket);
int bfm_gn_stats_rows(const void* rowsA, int nrowsA, int CA, const void* rowsB, int nrowsB, int CB, double weightB,
                      int64_t nvox, const float* gamma, const float* beta, int G, float eps, float* scale,
                      float* shift, float* bound, void* workspace, size_t workspace_bytes, void* ticket,
                      bfm_stream_t stream);
/* the same with the per-group mean / rstd kept for the backward pass (NULL: not wanted) */
int bfm_gn_stats_rows_train(const void* rowsA, int nrowsA, int CA, const void* rowsB, int nrowsB, int CB, double weightB,
                            int64_t nvox, const float* gamma, const float* beta, int G, float eps, float* scale,
                            float* shift, float* bound, float* mean_out, float* rstd_out, void* workspace,
                            size_t workspace_bytes, void* ticket, bfm_stream_t stream);

/* the same with each table given as rows [first, first + nrows) of a larger table of `total` rows: one sample's rows of a
 * batched producer ([S * nrows][C] planes, bfm_conv3x3x3_mfma_batch), read where they lie -- the first decoder above the
 * batched levels (buildingblocks.py:265-276: its upsampled source is one sample of the batch's output) */
int bfm_gn_stats_rows_sliced(const void* rowsA, int totalA, int firstA, int nrowsA, int CA, const void* rowsB, int totalB,
                             int firstB, int nrowsB, int CB, double weightB, int64_t nvox, const float* gamma,
                             const float* beta, int G, float eps, float* scale, float* shift, float* bound,
                             void* workspace, size_t workspace_bytes, void* ticket, bfm_stream_t stream);

/* Winograd F(4,3) along x (conv3d_wino4.hip): the same SingleConv body (buildingblocks.py:31-60) with 13.5 tap-rows
 * per output voxel instead of F(2,3)'s 18 -- dense boxes, one source, no split-K; rounding ~2x F(2,3)'s per layer
 * (2e-6 of max|y| against a float64 convolution), so it is a choice of the tune table, never the planner's default.
 * Weights packed by bfm_pack_conv_weights_wino4 (U = G g in float64); flags bit 0 = accumulate onto `out`;
 * moment_rows as elsewhere ([bfm_conv3x3x3_wino4_rows()][Cout]). */
size_t bfm_pack_conv_weights_wino4_bytes(int Cin, int Cout, int passes);
int bfm_pack_conv_weights_wino4(const float* w_oidhw, int Cin, int Cout, float wmax_abs_host, int passes, void* wpacked,
                                int* wexp_host, bfm_stream_t stream);
int bfm_conv3x3x3_wino4_rows(int D, int H, int W, int passes);
/* the (d,h,w) box of output voxels per workgroup for this volume: 8 x 8 x 4 (conv_wino4d: raw chunks by LDS-DMA one chunk
 * ahead, round 5) wherever the volume holds a full box in z and y, bfm_conv3x3x3_wino_box()'s otherwise */
int bfm_conv3x3x3_wino4_box(int D, int H, int W, int passes, int* box /* [3] */);
int bfm_conv3x3x3_wino4(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                        const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                        int flags, float* out, void* moment_rows /*or NULL*/, bfm_stream_t stream);
/* S same-shape samples in one launch (A (S,D,H,W,CA) -> out (S,D,H,W,Cout)): per-sample scale / shift rows affine_stride
 * apart (0 = CA), bound [S][G], moment_rows [S * bfm_conv3x3x3_wino4_rows()][Cout]; per sample the bits of
 * bfm_conv3x3x3_wino4.  The deep levels of same-shape tiles (buildingblocks.py:31-60 on a batch). */
int bfm_conv3x3x3_wino4_batch(const float* A, int CA, int S, int D, int H, int W, const float* scale, const float* shift,
                              const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                              int flags, float* out, void* moment_rows, int affine_stride, bfm_stream_t stream);
/* F(2,3) along x (bfm_conv3x3x3_wino_ex's arithmetic and weight pack, bfm_pack_conv_weights_wino) on boxes of 5 x 5 x 10
 * output voxels with a split K loop: the batched levels whose volumes are 5, 10 or 20 voxels wide, which no power-of-two
 * box divides (conv3d_wino_b5.hip).  Arguments as bfm_conv3x3x3_wino4_batch, plus a workspace of
 * bfm_conv3x3x3_wino_b5_workspace() bytes (16-byte aligned) for the K slabs, summed in slab order (no atomics); flags
 * bit 0 adds what `out` holds before LeakyReLU; moment_rows [S * bfm_conv3x3x3_wino_b5_rows()][Cout], one row per box, or
 * NULL.  Return codes as bfm_conv3x3x3_wino_ex, BFM_E_SHAPE unless D % 5 == 0, H % 5 == 0 and W % 10 == 0,
 * BFM_E_WORKSPACE for a short workspace.  The split factor (bfm_conv3x3x3_wino_b5_splitk; 0: shape not taken) depends on
 * the layer shape alone, never on S: a sample's workgroups do what they do in a launch of that sample alone. */
int bfm_conv3x3x3_wino_b5_rows(int D, int H, int W, int passes);
int bfm_conv3x3x3_wino_b5_splitk(int Cin, int Cout, int D, int H, int W);
size_t bfm_conv3x3x3_wino_b5_workspace(int Cin, int Cout, int S, int D, int H, int W);
int bfm_conv3x3x3_wino_b5_batch(const float* A, int CA, int S, int D, int H, int W, const float* scale, const float* shift,
                                const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                                int flags, float* out, void* moment_rows, int affine_stride, void* workspace,
                                size_t workspace_bytes, bfm_stream_t stream);
/* The masked form of bfm_conv3x3x3_wino4: the boxes (bfm_conv3x3x3_wino4_box) that hold a non-zero voxel of mask_image;
 * workspace bfm_conv3x3x3_wino4_masked_workspace(D, H, W, passes) bytes (4-byte aligned).  There
 * is no uniform-box pair: F(4,3)'s rounding reaches 4 voxels along x where F(2,3)'s numerical support is its
 * mathematical one (conv3d_wino4.hip), so the layers that take that shortcut stay with bfm_conv3x3x3_wino_uniform. */
size_t bfm_conv3x3x3_wino4_masked_workspace(int D, int H, int W, int passes);
/* The uniform-box pair of the F(4,3) kernel (round 5): bfm_conv3x3x3_wino_uniform's arguments and contract (flags from
 * bfm_uniform_boxes on the same box grid, same bits with and without them), for the layers whose output no other layer
 * that takes the shortcut reads -- the skip halves of the last two decoders' first convs (buildingblocks.py:265-276):
 * there a box's numerical support is its mathematical halo (a box is a whole number of quads).  BFM_E_SHAPE where the
 * volume's box differs from bfm_conv3x3x3_wino_box()'s.  scratch: bfm_conv3x3x3_wino4_uniform_scratch(Cout) bytes, 16-byte
 * aligned. */
size_t bfm_conv3x3x3_wino4_uniform_scratch(int Cout);
int bfm_conv3x3x3_wino4_uniform(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                                const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                                int flags, float* out, void* moment_rows, const unsigned char* uniform_flags, void* scratch,
                                bfm_stream_t stream);
/* the same, accumulating by need (flags == 3), for an `out` that a MASKED convolution on the same box grid reads next, with
 * keep_image (D,H,W) as its mask image: beside the class mates with `need`, the flagged boxes whose constant in keep_image is
 * not zero are stored -- the boxes that reader computes, and their neighbours, hold what a full launch stores. */
int bfm_conv3x3x3_wino4_uniform_keep(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                                     const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope,
                                     int passes, int flags, float* out, void* moment_rows, const unsigned char* uniform_flags,
                                     void* scratch, const float* keep_image, bfm_stream_t stream);
int bfm_conv3x3x3_wino4_masked(const float* A, int CA, int D, int H, int W, const float* scale, const float* shift,
                               const float* bound, int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                               int flags, float* out, const float* mask_image, void* workspace, size_t workspace_bytes,
                               bfm_stream_t stream);

size_t bfm_conv3x3x3_mfma_workspace(int Cin, int Cout, int D, int H, int W, int splitk);
int bfm_conv3x3x3_mfma_plan(int Cin, int Cout, int D, int H, int W, int* cfg_out /*[8]*/);
/* cfg[7] bit 0 ("accumulate"): add what `out` already holds before the LeakyReLU -- used for the skip half of a
 * decoder's first conv after bfm_conv3x3x3_upfold wrote the upsampled half. */

/* Decoder._joining + SingleConv (buildingblocks.py:265-276, 361-363), upsampled half only, for exact 2x nearest
 * upsampling (full-res dims == 2 x low-res dims): the 27 taps over the 8-fold replicated low-res tensor collapse to
 * 8 taps per output parity class with pre-summed weights (3.375x fewer FLOPs, the low-res box is what gets staged).
 * B [d][h][w][CB] low-res; scale_b/shift_b = the GroupNorm affine of channels CA.. of the concatenation; bound/G as
 * for _mfma; writes sum over (taps, B channels) WITHOUT activation to out [2d][2h][2w][Cout].  Follow with
 * bfm_conv3x3x3_mfma(A = skip, CB = 0, cfg[7] |= 1) on the skip channels' weights. */
size_t bfm_pack_conv_weights_upfold_bytes(int CB, int Cout, int passes);
int bfm_pack_conv_weights_upfold(const float* w_oidhw /*[Cout][CA+CB][27]*/, int CA, int CB, int Cout,
                                 float wmax_abs_host, int passes, void* wpacked, int* wexp_host, bfm_stream_t stream);
int bfm_conv3x3x3_upfold(const float* B, int CB, int d, int h, int w, const float* scale_b, const float* shift_b,
                         const float* bound, int G, const void* wpacked, int wexp, int Cout, int passes, float* out,
                         bfm_stream_t stream);
/* the same with split-K for low-res levels too small to fill the chip (workspace from _workspace(); 0 bytes = not needed):
 * partial sums per K slab, reduced in slab order */
size_t bfm_conv3x3x3_upfold_workspace(int CB, int d, int h, int w, int Cout);
int bfm_conv3x3x3_upfold_ex(const float* B, int CB, int d, int h, int w, const float* scale_b, const float* shift_b,
                            const float* bound, int G, const void* wpacked, int wexp, int Cout, int passes, float* out,
                            void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* S same-shape samples in one launch (the batched deep levels): B [S][d][h][w][CB], scale_b / shift_b [S][CB] (rows
 * affine_stride floats apart, 0 = CB: the upsampled half's window of the concat's [S][CA + CB] table), bound [S][G], out [S][2d][2h][2w][Cout].  A sample's result is bit-identical to its S = 1 launch: the
 * split-K plan depends on the per-sample shape alone, and a workspace smaller than _batch_workspace() is an error. */
size_t bfm_conv3x3x3_upfold_batch_workspace(int CB, int S, int d, int h, int w, int Cout);
int bfm_conv3x3x3_upfold_batch(const float* B, int CB, int S, int d, int h, int w, const float* scale_b,
                               const float* shift_b, const float* bound, int G, const void* wpacked, int wexp, int Cout,
                               int passes, float* out, void* workspace, size_t workspace_bytes, int affine_stride,
                               bfm_stream_t stream);

/* The smallest deep levels as tap-wise GEMMs on densely packed rows (conv3d_tap.hip).  X [S][n_lo][Cin] fp32 channels-last;
 * scale / shift [S][Cin] (rows affine_stride floats apart, 0 = Cin), bound [S][G] as for _upfold_batch.  wpacked: the
 * bfm_pack_conv_weights_mfma pack of a layer with kc_pack * 16 input channels, of which these Cin start at channel
 * kc_first * 16.  _tap_batch leaves P[tap][K slab][s * n_lo + v][Cout] = W[tap] . y[s][v] in the workspace;
 * bfm_tap_sum_batch (same Cin, Cout, S, n_lo, same workspace) then writes
 *   out[s][o][c] = (accumulate ? out : 0) + sum_tap sum_slab P[tap][slab][s * n_lo + table[o * 27 + tap]][c]
 * (taps and slabs ascending; table entry -1 = term dropped), optionally LeakyReLU(slope), optionally the moment rows of the
 * stored output: S * bfm_tap_sum_rows(n_hi, Cout) rows, laid out as bfm_moment_rows_bytes says.  A sample's bits do not
 * depend on S or on its place in the batch: the K slab plan is a function of (Cin, Cout) alone. */
size_t bfm_conv3x3x3_tap_batch_workspace(int Cin, int Cout, int S, int n_lo);
int bfm_conv3x3x3_tap_batch(const float* X, int Cin, int S, int n_lo, const float* scale, const float* shift,
                            const float* bound, int G, const void* wpacked, int wexp, int Cout, int kc_first, int kc_pack,
                            int passes, void* workspace, size_t workspace_bytes, int affine_stride, bfm_stream_t stream);
int bfm_tap_sum_rows(int n_hi, int Cout);
int bfm_tap_sum_batch(const void* workspace, int Cin, int Cout, int S, int n_lo, const int* table /*[n_hi][27], device*/,
                      int n_hi, float slope, int activation, int accumulate, float* out, void* moment_rows /*or NULL*/,
                      bfm_stream_t stream);

int bfm_conv3x3x3_mfma(const float* A, int CA, const float* B, int CB, int D, int H, int W,
                       const bfm_upsample_t* up, const float* scale, const float* shift, const float* bound,
                       int G, const void* wpacked, int wexp, int Cout, float slope, int passes,
                       const int* cfg /*from _plan, or NULL*/, float* out, void* workspace,
                       size_t workspace_bytes, bfm_stream_t stream);

/* ------------------------------------------------------------- MaxPool3d(2)
 * nn.MaxPool3d(kernel_size=2): stride 2, floor, no padding
 * (buildingblocks.py:185-186).  in (D,H,W,C) -> out (D/2,H/2,W/2,C). */
int bfm_maxpool2(const float* in, int C, int D, int H, int W, float* out, bfm_stream_t stream);

/* ------------------------------------------------------------------- tail
 * Everything after the last decoder, one pass over the 64-ch feature map:
 * F.normalize(dim=1) (unet3d/model.py:207-208) -> TaskHead 1x1x1 convs + bias
 * (head.py:52-59) -> SegProcessor softmax / DistProcessor clamp
 * (joiner.py:69-77,149-157) -> get_postprocessor (Trainer/models/__init__.py:
 * 272-354): exp, tanh cortical formula, LUT[argmax], CT*1000, residual+input.
 * The head set is data: `roles[o]` gives the meaning of head output row o. */
enum {
    BFM_ROLE_PLAIN = 0,     /* write as is (T1, T2, FLAIR, regx/y/z, high_res_residual, *_sigma) */
    BFM_ROLE_CT = 1,        /* x1000 */
    BFM_ROLE_BIAS_LOG = 2,  /* exp */
    BFM_ROLE_SEG = 3,       /* softmax member (contiguous run of n_seg rows) */
    BFM_ROLE_DIST = 4,      /* clamp(+-max_dist) as fminf(fmaxf(v, -max_dist), max_dist): a NaN logit comes out as
                               -max_dist, where torch.clamp keeps the NaN; order lp, lw[, rp, rw] */
    BFM_ROLE_SR = 5,        /* high_res_residual: also emits high_res = v + input */
    BFM_ROLE_PATHOL = 6     /* sigmoid */
};
typedef struct {
    int n_out;                  /* rows of head_w (sum of head channels) */
    int c_feat;                 /* 64 */
    const float* head_w;        /* [n_out][c_feat] */
    const float* head_b;        /* [n_out] */
    const int32_t* roles;       /* [n_out] BFM_ROLE_* */
    const int32_t* out_slot;    /* [n_out] index into `maps` for this row, -1 = none */
    int seg_first, n_seg;       /* rows of the segmentation head; n_seg==0 -> none */
    const int32_t* seg_lut;     /* [n_seg] label list */
    int n_dist;                 /* 0, 2 (left hemi) or 4 */
    int dist_first;
    float max_dist;
    int unit_feat;              /* apply F.normalize before the heads */
    int slot_high_res;          /* maps slot for residual+input, -1 = none; a residual head with c channels (rows with
                                   BFM_ROLE_SR, contiguous) writes channel j to slot_high_res + j */
    int slot_fake_cortical;     /* maps slot, -1 = none */
    int n_maps;                 /* length of the `maps` pointer array (every out_slot / slot_* is < n_maps) */
    float head_wmax;            /* max |head_w| (host knows it): > 0 with unit_feat selects the split-f16 matrix-core
                                   path (fp32-grade, like conv3x3x3_mfma); 0 keeps the exact fp32 MFMA chain */
    int skip_zero_input;        /* 1: a run of 64 voxels whose `input` is all zero is not evaluated (its maps / label stay
                                   unwritten).  For the tile loop only, which keeps outputs where the tile's input is
                                   non-zero (scripts/demo_test.py:88-100); evaluate_image always passes 0 */
} bfm_tail_desc_t;

int bfm_tail_heads(const float* feat, const float* input /*[nvox], may be NULL*/, int64_t nvox,
                   const bfm_tail_desc_t* desc, float* feat_norm /*[nvox][c_feat] or NULL*/,
                   float* const* maps /*device array of device pointers, each [nvox]*/,
                   float* seg_prob /*[nvox][n_seg] or NULL*/, int64_t* label /*[nvox] or NULL*/,
                   float* raw_out /*[nvox][n_out]: if set, write raw head logits only (TaskHead.forward)*/,
                   bfm_stream_t stream);
/* The same pass writing its maps into the rows of ONE buffer: map i = maps_rows + i * row_stride (row_stride >= nvox
 * floats), so a caller that allocates the maps together needs no device-side pointer table (the tile loop inside a
 * hipGraph: no table-building kernels).  flags bit 0 = skip_zero_input for this call (see bfm_tail_desc_t; the
 * descriptor itself stays the one evaluate_image uses).  Replaces the same reference lines as bfm_tail_heads. */
int bfm_tail_heads_rows(const float* feat, const float* input /*[nvox], may be NULL*/, int64_t nvox,
                        const bfm_tail_desc_t* desc, float* feat_norm /*or NULL*/, float* maps_rows, int64_t row_stride,
                        float* seg_prob /*or NULL*/, int64_t* label /*or NULL*/, int flags, bfm_stream_t stream);
/* Host arithmetic, no device needed: the instantiation of the tail kernel that a call with this descriptor takes (the
 * launcher dispatches on it).  0 = fp32 MFMA chain (unit_feat == 0, head_wmax not a finite positive number, or
 * c_feat % 16 != 0), 1 = split-f16 generic, 2 = split-f16 with 56 classes and 3 column blocks (65..96 outputs: the shipped
 * head set), 3 = split-f16 with 18 classes and 1 column block (the left-hemisphere head set).  -1 for NULL. */
int bfm_tail_route(const bfm_tail_desc_t* desc);

/* ----------------------------------------------------------------- stitch
 * scripts/demo_test.py:88-119 without the NIfTI round trip:
 *   full[k][range] += tile[k] * (tile_input != 0)   then   full[k] /= cnt.
 * tile maps are [td*th*tw] fp32 (or int64 labels, summed as float like the
 * reference, quirk Q5). */
int bfm_stitch_accumulate(const float* tile, const int64_t* tile_label, const float* tile_input,
                          int td, int th, int tw, float* full, int D, int H, int W,
                          int z0, int y0, int x0, bfm_stream_t stream);
/* All K stitched keys of one tile in one launch: maps [n_maps][td*th*tw] (row stride map_stride), sel[k] = map
 * row feeding key k or -1 for the int64 label, full [K][D*H*W].  tile_input == NULL: the rows are already masked
 * and float typed (what bfm_pack_tile_multi produced on a peer rank); sel must then be >= 0. */
int bfm_stitch_accumulate_multi(const float* maps, int64_t map_stride, const int32_t* sel, int K,
                                const int64_t* tile_label, const float* tile_input, int td, int th, int tw, float* full,
                                int D, int H, int W, int z0, int y0, int x0, bfm_stream_t stream);
/* tile_input == NULL in bfm_stitch_accumulate means "already masked". */
int bfm_tile_count_add(float* cnt, int D, int H, int W, int z0, int z1, int y0, int y1, int x0, int x1,
                       bfm_stream_t stream);
/* the K keys of one tile, masked (x tile_input != 0) and float typed, packed [K][n]: the multi-GPU shipping form */
int bfm_pack_tile_multi(const float* maps, int64_t map_stride, const int32_t* sel, int K, const int64_t* tile_label,
                        const float* tile_input, int64_t n, float* out, bfm_stream_t stream);
/* full [K][vol] /= cnt [vol], one launch */
int bfm_divide_by_count_multi(float* full, const float* cnt, int64_t vol, int K, bfm_stream_t stream);
/* The whole stitch in one launch once every tile's packed rows ([K][td*th*tw], bfm_pack_tile_multi) are resident on
 * one device -- rank 0 of the multi-GPU path, scripts/demo_test.py:108-119: full[k][v] = (0 + sum over the tiles
 * covering v, in table order) / (their number), each voxel written once.  tiles: device table [T][8] int64 =
 * {device pointer to the tile's rows, z0, y0, x0, td, th, tw, 0} in the reference's tile order; T <= 2048.
 * Bit-identical to T x bfm_stitch_accumulate_multi on a zeroed volume + bfm_divide_by_count_multi. */
int bfm_stitch_gather_multi(const int64_t* tiles, int T, int K, float* full, int D, int H, int W, bfm_stream_t stream);

/* The compact shipping form of the same flow.  scripts/demo_test.py:88-100 keeps tile_output * (tile input != 0), and a
 * tile's input is a window of the volume: which voxels of a tile survive is known from the volume alone, on every rank,
 * before any tile is computed.  A tile's K rows then hold its surviving voxels only, in the tile's raster order:
 * rows [K][row_stride], voxel i of the tile at column pos[i] = the number of non-zero input voxels before i in the tile.
 *   bfm_tile_mask_index: pos[] of every tile and nnz[t] = its number of surviving voxels, three launches per volume.
 *     tiles: device table [T][8] int64 = {offset of the tile's first entry in pos[], z0, y0, x0, td, th, tw, first block},
 *     first block = sum of bfm_tile_mask_blocks(td*th*tw) over the tiles before it, total_blocks = that sum over all
 *     tiles; block_ws: total_blocks int32 of scratch.
 *   bfm_pack_tile_compact: bfm_pack_tile_multi writing the surviving voxels only (row_stride >= the tile's nnz).
 *   bfm_stitch_gather_compact: bfm_stitch_gather_multi reading such rows; tiles [T][10] int64 = {rows, the tile's pos,
 *     z0, y0, x0, td, th, tw, row_stride, 0}, volume = the (D,H,W) input the masks come from; T <= 1024.
 * Results are bit-identical to the dense form (a masked-out voxel adds +0 in every tile). */
int bfm_tile_mask_blocks(int64_t tile_voxels);
int bfm_tile_mask_index(const float* volume, int D, int H, int W, const int64_t* tiles, int T, int total_blocks,
                        int32_t* pos, int32_t* nnz, int32_t* block_ws, bfm_stream_t stream);
int bfm_pack_tile_compact(const float* maps, int64_t map_stride, const int32_t* sel, int K, const int64_t* tile_label,
                          const float* tile_input, int64_t n, const int32_t* pos, int64_t row_stride, float* out,
                          bfm_stream_t stream);
int bfm_stitch_gather_compact(const int64_t* tiles, int T, int K, const float* volume, float* full, int D, int H, int W,
                              bfm_stream_t stream);

/* ------------------------------------------------------------ elementwise
 * Per-voxel helpers for the stand-alone processors / post-processor
 * (joiner.py:69-77,149-157; Trainer/models/__init__.py:272-354) and the
 * synthesis augmentations (Generator/utils.py:568-638).  Strides are in
 * elements so channel slices of channels-last buffers are read in place. */
enum {
    BFM_EW_EXP = 0, BFM_EW_AFFINE = 1 /* x*a+b */, BFM_EW_CLAMP = 2 /* [a,b]; NaN -> a (fmaxf) */, BFM_EW_CLAMP_MIN = 3,
    BFM_EW_GAMMA = 4 /* a*(x/a)^b, add_gamma_transform utils.py:568-572 */, BFM_EW_SIGMOID = 5,
    BFM_EW_DIV = 6 /* x/a */, BFM_EW_NONZERO = 7 /* x!=0 ? 1:0 */, BFM_EW_SUB_DIV = 8 /* (x-a)/b */,
    BFM_EW_GE = 9 /* x>=a ? 1:0, binarize utils.py:65-72 */,
    BFM_EW_NAN_TO_NUM = 10 /* torch.nan_to_num defaults, utils/test_utils.py:239 */
};
enum {
    BFM_EW_ADD = 0, BFM_EW_MUL = 1, BFM_EW_MUL_EXP = 2 /* x*exp(y), add_bias_field utils.py:585-587 */,
    BFM_EW_AXPY_CLAMP0 = 3 /* max(x+a*y,0), add_noise utils.py:633-638 */, BFM_EW_AXPY = 4, BFM_EW_DIV2 = 5,
    BFM_EW_ZERO_WHERE_ZERO = 6 /* y==0 ? 0 : x, target['pathology'][SYN_cerebral == 0] = 0, datasets.py:398-399 */
};
int bfm_ew_unary(int op, const float* in, int64_t in_stride, float* out, int64_t out_stride, int64_t n,
                 float a, float b, bfm_stream_t stream);
int bfm_ew_binary(int op, const float* x, int64_t x_stride, const float* y, int64_t y_stride /*0 = broadcast*/,
                  float* out, int64_t out_stride, int64_t n, float a, bfm_stream_t stream);
/* max |x| over `rows` runs of `len` floats `row_stride` apart, folded into *out_zeroed (device, +0 on entry) by an integer
 * atomic maximum of the bit pattern: the max |w| the weight packers scale by, one launch per layer without a host round
 * trip each (training re-packs every layer after AdamW: round 3 used four torch kernels per layer for it). */
int bfm_absmax_f32(const float* x, int64_t rows, int64_t len, int64_t row_stride, float* out_zeroed, bfm_stream_t stream);
int bfm_softmax_cl(const float* x, int64_t x_row_stride, int C, float* y, int64_t y_row_stride, int64_t n,
                   bfm_stream_t stream);
/* The backward of the per-voxel processors for losses written in torch (brainfm_amd/autograd.py): what torch autograd
 * derives from joiner.py:69-77 (softmax), :79-87 (sigmoid) and :149-157 (clamp).
 * bfm_softmax_cl_bwd: dx[i][c] = p[i][c] * (g[i][c] - sum_j p[i][j] g[i][j]) from the stored posterior p; rows of C floats
 * `*_row_stride` apart (views of wider buffers are read in place), one thread per row as bfm_softmax_cl, the sum taken in
 * channel order in fp32.  dx overlaps neither p nor g.
 * bfm_ew_unary_bwd: BFM_EW_SIGMOID reads the OUTPUT y: dx = g * y * (1 - y); BFM_EW_CLAMP reads the INPUT x: dx = g where
 * a <= x <= b (both edges inclusive, as torch.clamp's backward), 0 elsewhere and for a NaN x.  Other ops: BFM_E_ARG.
 * Strides in elements, as bfm_ew_unary. */
int bfm_softmax_cl_bwd(const float* p, int64_t p_row_stride, const float* g, int64_t g_row_stride, int C, float* dx,
                       int64_t dx_row_stride, int64_t n, bfm_stream_t stream);
int bfm_ew_unary_bwd(int op, const float* x_or_y, int64_t stride, const float* g, int64_t g_stride, float* dx,
                     int64_t dx_stride, int64_t n, float a, float b, bfm_stream_t stream);
/* out[i] = lut[first maximum of row i] (lut NULL: the index).  A NaN is never greater than anything, so a row holding a NaN
 * gives the first maximum of its other members, unless the NaN is in column 0, which then stays the maximum: torch.argmax
 * picks a NaN, and this kernel does not unless it is in column 0.  The inference flow only sees all-NaN rows, where both
 * give 0. */
int bfm_argmax_lut_cl(const float* p, int64_t row_stride, int C, const int32_t* lut, int64_t* out, int64_t n,
                      bfm_stream_t stream);
int bfm_fake_cortical(const float* dist, int64_t row_stride, int n_dist, float* out, int64_t n,
                      bfm_stream_t stream);
/* Stage-1 input of the two-stage (inpainting) model in one pass: out[v] = { x[v] * (1 - p[v]), p[v] }, channels-last
 * [n][2] (utils/test_utils.py:336-338: samples[i]['input'] * (1 - outputs_pathol[i]['pathology']), then joiner.py's
 * torch.concat([x, cond], dim=1)).  1 - p and the product are two fp32 roundings, bit-equal to torch.  out 8-byte aligned. */
int bfm_mask_concat2(const float* x, const float* p, int64_t n, float* out, bfm_stream_t stream);
/* The input of a mask-conditioned network in training, in one pass (Trainer/engine.py:102-112: samples[i]['input'] *=
 * 1 - target['pathology'], torch.flip(samples[i]['input'], dims=[2]) and the concat of the condition channels; then
 * joiner.py:178's torch.concat([x, cond], dim=1) and the channels-last repack).  x, p: (D,H,W) volumes.
 *   mode 0 'mask'       out [D][H][W][2] = { m, p }               m = x * (1 - p), two fp32 roundings as in torch
 *   mode 1 'flip'       out [D][H][W][2] = { x, x[D-1-d] }        (p unused, may be NULL)
 *   mode 2 'mask+flip'  out [D][H][W][3] = { m, m[D-1-d], p }     the flip is of the masked input, first spatial axis
 * masked / flipped (each may be NULL): m and the flipped image as (D,H,W) volumes -- what the reference leaves in
 * samples[i]['input'] and samples[i]['input_flip'].  Bit-equal to the torch expressions.  Must not alias x or p. */
int bfm_condition_input(const float* x, const float* p, int mode, int D, int H, int W, float* out, float* masked,
                        float* flipped, bfm_stream_t stream);
/* The stage-1 input of the two-stage model in training, in one pass (Trainer/engine.py:230-243: PatholProcessor's sigmoid,
 * joiner.py:79-87; samples[i]['input_masked'] = samples[i]['input'] * (1 - outputs_pathol[i]['pathology']); cond =
 * target['pathology']; joiner.py:178's concat).  raw0 of voxel v is raw0[col_offset + v * voxel_stride] (bfm_loss_pathol's
 * addressing).  p_out [n] = sigmoid(raw0) = 1 / (1 + expf(-raw0)), the expression bfm_loss_pathol evaluates, so the loss and
 * the mask see the same p; out [n][2] = { x * (1 - p), t }, two fp32 roundings as in torch; t NULL: a zero mask.
 * masked_out [n] (may be NULL): x * (1 - p) as a volume (samples[i]['input_masked']).  out 8-byte aligned. */
int bfm_twostage_train_input(const float* x, const float* raw0, int64_t col_offset, int64_t voxel_stride, const float* t,
                             int64_t n, float* out /*[n][2]*/, float* p_out /*[n]*/, float* masked_out /*[n] or NULL*/,
                             bfm_stream_t stream);

/* ---------------------------------------------------------------- synthesis
 * Gather / resample kernels of Generator/utils.py and utils/interpol (fp32, results bit-identical to the
 * reference's CPU path where it is a fixed sequence of IEEE operations).  Volumes are (nx,ny,nz[,C])
 * row-major with channels last, exactly the reference's layout. */
/* fast_3D_interp_torch(X, II, JJ, KK, 'linear', default) -- Generator/utils.py:140-192: valid iff
 * II>0 && II<=nx-1 (strict lower bound), upper corner clamped, invalid -> default_value. */
int bfm_interp3d_linear(const float* X, int nx, int ny, int nz, int C, const float* II, const float* JJ,
                        const float* KK, int64_t n, float default_value, float* out, bfm_stream_t stream);
/* ... 'nearest' -- :124-138: round half to even, clamp; 4-byte elements copied bitwise (int32 or fp32). */
int bfm_interp3d_nearest(const void* X, int nx, int ny, int nz, int C, const float* II, const float* JJ,
                         const float* KK, int64_t n, void* out, bfm_stream_t stream);
/* get_deformed_atlas -- utils/test_utils.py:45-57, fused: where mask>0, sample the atlas trilinearly at
 * A(3x4) applied to 100*(regx,regy,regz); 0 elsewhere. */
int bfm_deformed_atlas(const float* mask, const float* regx, const float* regy, const float* regz, const float* atlas,
                       int nx, int ny, int nz, const float* A_host, int64_t n, float* out, bfm_stream_t stream);
/* The same inside the tile loop -- scripts/demo_test.py:88-89,102-104: the mask operand is the tile's input image and
 * M = (tile_in != 0), i.e. the 0/1 mask the script builds before it calls get_deformed_atlas.  Both entry points read
 * the atlas with L1-bypassing (sc1) loads: see HISTORY.md section 3.3. */
int bfm_deformed_atlas_tile(const float* tile_in, const float* regx, const float* regy, const float* regz,
                            const float* atlas, int nx, int ny, int nz, const float* A_host, int64_t n, float* out,
                            bfm_stream_t stream);
/* myzoom_torch -- Generator/utils.py:200-257.  Per-axis tables (floor index, ceil index, weights) are built
 * by the host exactly as the reference builds them (torch.arange in fp32); the three passes are fused. */
typedef struct { const int32_t* f; const int32_t* c; const float* wf; const float* wc; } bfm_zoom_axis_t;
int bfm_zoom_linear(const float* X, int nx, int ny, int nz, int C, const bfm_zoom_axis_t* axes /*[3]*/, int ox, int oy,
                    int oz, float* out, bfm_stream_t stream);
/* Which kernel bfm_zoom_linear runs for these extents (host arithmetic, no device needed; the launcher asks here too):
 * 0 = the whole source in LDS, 1 = wave rows in LDS with 16-byte stores, 2 = the same with scalar stores, 3 = per output
 * element for long rows.  out_aligned16: whether the output pointer is 16-byte aligned.  < 0: BFM_E_ARG / BFM_E_SHAPE. */
int bfm_zoom_linear_route(int nx, int ny, int nz, int C, int ox, int oy, int oz, int out_aligned16);
/* one axis of gaussian_blur_3d -- Generator/utils.py:84-94: zero-padded 1-D correlation, odd kernel. */
int bfm_conv1d_axis(const float* in, int nx, int ny, int nz, int axis, const float* kern, int klen, float* out,
                    bfm_stream_t stream);
/* The launch bfm_conv1d_axis makes (host arithmetic, no device needed; the launcher asks here too): 0 / 1 / 2 = the LDS
 * slab kernel of that axis, 3 = the per-tap fallback (klen > 64, or axis 2 with nz > 1024).  seg: outputs along the
 * filtered axis (axes 0, 1) or rows (axis 2) per slab, 0 for the fallback; nslab: workgroups; lds_bytes: dynamic LDS.
 * Each of the three may be NULL.  < 0: BFM_E_ARG / BFM_E_SHAPE. */
int bfm_conv1d_axis_plan(int nx, int ny, int nz, int axis, int klen, int* seg, int* nslab, size_t* lds_bytes);
/* interpol.grid_push / grid_grad (order 1, 3-D) -- utils/interpol/iso1.py:136-387; with grid_pull they make
 * grid_pull / grid_push differentiable to first order (autograd.py:125-190, pushpull.py:262-310).
 * push: inp (Bi,C,ix,iy,iz) scattered through grid (Bg,ix,iy,iz,3) into out (B,C,nx,ny,nz), which MUST be zero on
 * entry (fp32 atomics).  grad: out (B,C,ox,oy,oz,3). */
int bfm_grid_push3d_linear(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx,
                           int ny, int nz, const int* bound, int extrapolate, float* out_zeroed, bfm_stream_t stream);
int bfm_grid_grad3d_linear(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                           int oy, int oz, const int* bound, int extrapolate, float* out, bfm_stream_t stream);

/* The window a tile takes of the volume (scripts/demo_test.py:84-86, `full_im[:, :, x0:x1, y0:y1, z0:z1]`), copied into
 * a contiguous [d][h][w] buffer: vol [D][H][W] fp32, the window starts at (z0, y0, x0) in that index order. */
int bfm_crop3d(const float* vol, int D, int H, int W, int z0, int y0, int x0, int d, int h, int w, float* out,
               bfm_stream_t stream);

/* Pre-processing around the inference path (utils/test_utils.py:235-284 prepare_image).
 * permute_flip3d: align_volume_to_ref's swapaxes + flips (utils/misc.py:1207-1247) in one gather:
 *   out dims = (n[perm[0]], n[perm[1]], n[perm[2]]); out[i0,i1,i2] = in[j], j[perm[a]] = flip[a] ? n[perm[a]]-1-ia : ia.
 * bbox_nonzero: zero_crop's torch.argwhere(x > tol) min/max (utils/test_utils.py:60-72): box[6] = {x0,y0,z0,x1,y1,z1}
 *   (x1 exclusive); all-background volumes give x0 > x1.
 * mean_lastdim: im.mean(dim=-1) for multi-frame inputs (utils/test_utils.py:243). */
int bfm_permute_flip3d(const float* in, int nx, int ny, int nz, const int* perm /*[3] host*/,
                       const int* flip /*[3] host*/, float* out, bfm_stream_t stream);
int bfm_bbox_nonzero(const float* in, int nx, int ny, int nz, float tol, int32_t* box /*[6] device*/,
                     bfm_stream_t stream);
int bfm_mean_lastdim(const float* in, int64_t n, int c, float* out, bfm_stream_t stream);

/* interpol.resize(interpolation=3, prefilter=True) -- utils/interpol/resize.py:13-119, coeff.py:254-344, nd.py:36-142
 * (Generator/datasets.py:337-338, `bspline_zooming`).  One axis at a time, in place for the prefilter.
 * prefilter: bound 1 ('nearest') or 3 ('dct2') -> DCT-II conditions; the host passes the scalars the reference derives
 * from the pole z = sqrt(3)-2 (gain (1-z)(1-1/z), pole_last, init_scale z/(1-z^2n), final_scale z/(z-1)) and the
 * fp32 table init_w[i-1] = z^i + z^(2n-1-i), i = 1..n-2.  resample: out[o] = sum of 4 cubic B-spline taps around
 * coord[o] (fp32 source coordinates of the output samples along `axis`), indices reflected (3) or clamped (1).
 * The prefilter also serves interpol.spline_coeff_nd for order 2 (pole sqrt(8)-3, coeff.py:35-57) and the other two
 * families of conditions the reference has (coeff.py:229-251); max_iter = ceil(-30 / log|z|) (coeff.py:72, :99):
 *   bound 0 ('zero') or 2 ('dct1') -> DCT-I (coeff.py:96-140, 207-214): pole_last = z^(n-1),
 *     init_scale = 1/(1-z^(2n-2)) (used when max_iter >= n), final_scale = z/(z^2-1); init_w unused;
 *   bound 6 ('dft') -> DFT (coeff.py:69-95, 181-205): with m = min(max_iter, n), init_scale = 1/(1-z^m),
 *     final_scale = 1/(z^m-1); init_w and pole_last unused.
 * bound 4 / 5 ('dst1' / 'dst2') -> BFM_E_SHAPE: the reference has no prefilter for them. */
int bfm_bspline3_prefilter_axis(float* vol, int nx, int ny, int nz, int axis, int bound, float pole, float gain,
                                const float* init_w, float pole_last, float init_scale, float final_scale,
                                int max_iter, bfm_stream_t stream);
int bfm_bspline3_resample_axis(const float* in, int nx, int ny, int nz, int axis, const float* coord, int n_out,
                               int bound, float* out, bfm_stream_t stream);

/* interpol.grid_pull(interpolation='linear') -> iso1.pull3d -- utils/interpol/iso1.py:28-133.
 * inp (Bi,C,nx,ny,nz), grid (Bg,ox,oy,oz,3), out (max(Bi,Bg),C,ox,oy,oz); bound[3] in 0..6
 * (zero, replicate, dct1, dct2, dst1, dst2, dft -- bounds.py:8-15); extrapolate 0 no / 1 yes / 2 hist. */
int bfm_grid_pull3d_linear(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                           int oy, int oz, const int* bound, int extrapolate, float* out, bfm_stream_t stream);
/* interpol.grid_pull / grid_push / grid_grad for spline orders 0 to 3, any order per axis -> nd.pull / nd.push /
 * nd.grad -- utils/interpol/nd.py:30-290, splines.py:30-43 and :90-103, bounds.py:24-89.  The arguments of the _linear
 * exports plus order[3], each 0..3 (BFM_E_ARG otherwise): per axis grid0 = floor(g - (order-1)/2), node k in 0..order
 * at bound_index(grid0+k) with bound_sign(grid0+k) and weight fastweight(g - grid0 - k); grad takes fastgrad on its
 * own axis.  push: out MUST be zero on entry (fp32 atomics).  order {1,1,1} follows nd.py here, whose gradient on a
 * linear axis has the sign of splines.py:93-97; the _linear exports follow iso1.py. */
int bfm_grid_pull3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                           int oy, int oz, const int* bound, const int* order, int extrapolate, float* out,
                           bfm_stream_t stream);
int bfm_grid_push3d_spline(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx,
                           int ny, int nz, const int* bound, const int* order, int extrapolate, float* out_zeroed,
                           bfm_stream_t stream);
int bfm_grid_grad3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                           int oy, int oz, const int* bound, const int* order, int extrapolate, float* out,
                           bfm_stream_t stream);
/* The same three on 2-D grids -> iso0.pull2d / push2d (iso0.py) for order {0,0}, iso1.pull2d / push2d / grad2d (iso1.py)
 * for order {1,1}, nd.pull / nd.push / nd.grad (nd.py:30-290) for every other combination.  inp (Bi,C,nx,ny), grid
 * (Bg,ox,oy,2), out (max(Bi,Bg),C,ox,oy), grad out (B,C,ox,oy,2); bound[2] and order[2] are read, checked as above.
 * push: out MUST be zero on entry (fp32 atomics).  grad at order {1,1} takes iso1's slope (-1 / +1); a linear axis of a
 * mixed-order call takes the sign of splines.py:93-97, as in 3-D.  Serves the autograd of grid_pull / grid_push. */
int bfm_grid_pull2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox, int oy,
                           const int* bound, const int* order, int extrapolate, float* out, bfm_stream_t stream);
int bfm_grid_push2d_spline(const float* inp, int Bi, int C, int ix, int iy, const float* grid, int Bg, int nx, int ny,
                           const int* bound, const int* order, int extrapolate, float* out_zeroed, bfm_stream_t stream);
int bfm_grid_grad2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox, int oy,
                           const int* bound, const int* order, int extrapolate, float* out, bfm_stream_t stream);
/* interpol.grid_hess / grid_pushgrad, the two halves of the backward of grid_grad (utils/interpol/pushpull.py:176-233 and
 * :303-325) -> nd.hess / nd.pushgrad (nd.py:291-464), iso1.hess3d / pushgrad3d for order {1,1,1} (iso1.py:390-675) and
 * the zeros of iso0.hess / pushgrad for order {0,0,0} (iso0.py:326-368).  One export per operation takes every order and
 * dispatches inside; the nodes, signs, weights, mask and argument checks are those of the _spline exports above.
 * hess: entry (d,d) takes fasthess (splines.py:149-157) on axis d, entry (d,d2) fastgrad on both axes, the lower
 *   triangle mirrors the upper one, and the inbounds mask multiplies the result for every B and C (nd.py:456 raises, or
 *   returns a wrong shape, unless B = C = 1, where it gives this product).  cot NULL: out (B,C,ox,oy,oz,3,3).  cot
 *   (B,C,ox,oy,oz,3), B = max(Bi,Bg): out (B,ox,oy,oz,3), out[b,v,j] = sum_c sum_i hess[b,c,v,i,j] * cot[b,c,v,i] --
 *   pushpull.py:322-324 without the Hessian in memory.  Every element of out is written.
 * pushgrad: inp (Bi,C,ix,iy,iz,3) scattered through grid (Bg,ix,iy,iz,3) into out (B,C,nx,ny,nz), which MUST be zero on
 *   entry: node by node sign * mask * (c_x dwx wy wz + c_y wx dwy wz + c_z wx wy dwz), one fp32 atomic each.
 * Order {1,1,1} takes iso1's slope (-1 / +1), the opposite of the generic path's fastgrad on a linear axis of a
 * mixed-order call: the same Hessian, the opposite sign for pushgrad. */
int bfm_grid_hess3d(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox, int oy,
                    int oz, const int* bound, const int* order, int extrapolate, const float* cot, float* out,
                    bfm_stream_t stream);
int bfm_grid_pushgrad3d(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx, int ny,
                        int nz, const int* bound, const int* order, int extrapolate, float* out_zeroed,
                        bfm_stream_t stream);
/* Bit-reproducible forms of the four scatter exports above: bfm_grid_push3d_spline_fixed replaces bfm_grid_push3d_spline,
 * bfm_grid_push2d_spline_fixed bfm_grid_push2d_spline, bfm_grid_push3d_linear_fixed bfm_grid_push3d_linear and
 * bfm_grid_pushgrad3d_fixed bfm_grid_pushgrad3d where the same bits are wanted on every run.  Each takes its sibling's
 * arguments and a workspace of bfm_grid_push_fixed_workspace(B, C, nx*ny*nz) bytes (B = max(Bi,Bg); 0 for a bad
 * argument) before the stream; `out` need NOT be zero on entry and every element of it is written.  The kernels, nodes,
 * weights and contributions are the sibling's; only the accumulation differs.  Per slice (b, c) of inp: m = max |inp|
 * over the slice (pushgrad: over its 3 components too), taken on the device; e with m < 2^e (frexp); bits =
 * bfm_grid_push_fixed_bits(P, order, D, G) = ceil(log2(P * T * G)) with P = the grid points of a batch item, T = the
 * product of order[a] + 1 over the D axes and G = 1 (push) or 3 (pushgrad), a bound of |contribution| / m; k = 62 - bits -
 * e.  A contribution c, the fp32 value the sibling adds, goes as q = rint(c * 2^k) (nearest even, exact in double) into
 * an int64 accumulator with one 64-bit integer atomic, so the sum has no order and cannot overflow; then out =
 * (float)((double)acc * 2^-k).  m = 0: the slice is +0.  m NaN or Inf (pushgrad: or 2^126 and more, where 3 m need not be
 * a finite float): the whole slice is NaN (the siblings poison the touched nodes only), other slices are unaffected.
 * bits > 40 (or P, order, D, G out of range): BFM_E_ARG.  No host read-back; everything runs on `stream`. */
int bfm_grid_push_fixed_bits(int64_t P, const int* order, int D, int G);
size_t bfm_grid_push_fixed_workspace(int B, int C, int64_t nvox);
int bfm_grid_push3d_spline_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx,
                                 int ny, int nz, const int* bound, const int* order, int extrapolate, float* out,
                                 void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_grid_push2d_spline_fixed(const float* inp, int Bi, int C, int ix, int iy, const float* grid, int Bg, int nx, int ny,
                                 const int* bound, const int* order, int extrapolate, float* out, void* workspace,
                                 size_t workspace_bytes, bfm_stream_t stream);
int bfm_grid_push3d_linear_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx,
                                 int ny, int nz, const int* bound, int extrapolate, float* out, void* workspace,
                                 size_t workspace_bytes, bfm_stream_t stream);
int bfm_grid_pushgrad3d_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg, int nx,
                              int ny, int nz, const int* bound, const int* order, int extrapolate, float* out,
                              void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* interpol.restrict -- utils/interpol/restrict.py:9-122 (grid_push, nd.py:148-214, on torch.stack(meshgrid_ij(*lin))) --
 * and the backward of the separable cubic interpol.resize, as per-axis sparse operators.  A separable grid has one
 * coordinate list per axis, so the (order+1)^3 taps of nd.py factor into three axis passes.
 * axis_table: the operator of coord[m] (fp32, device) against an axis of n nodes as a CSR table: coordinate i touches
 *   node k = 0..order at bound_index(g0+k) with value fastweight(g - g0 - k) * bound_sign(g0+k) * mask_i, the nodes and
 *   the inbounds mask of the _spline exports above, the mask taken against this axis alone.  transpose 0 (pull
 *   direction): m rows of order+1 entries, rowptr[m+1].  transpose 1 (push direction): n rows, rowptr[n+1], the entries
 *   of a row in ascending (i, k), entries that are exactly 0 left out.  col / val hold m * (order+1) entries either way;
 *   the transposed build needs bfm_spline_axis_table_workspace bytes (BFM_E_WORKSPACE otherwise).
 *   ties_even 1 (order 0 only; 0 / 1, BFM_E_ARG otherwise): the node is round(g) with a tie to the even node, what
 *   iso0.py:12 computes when all three orders of a call are 0, instead of floor(g + 0.5) of nd.py:45.
 *   order 0..3, bound 0..6, extrapolate 0..2 (BFM_E_ARG otherwise); m, n <= 2^24 (BFM_E_SHAPE otherwise).
 * axis_pass: in (lead,nx,ny,nz) -> out with the length of `axis` replaced by n_out, all lead volumes in one launch:
 *   out[.., r, ..] = sum over e in rowptr[r]..rowptr[r+1]-1, ascending, of val[e] * in[.., col[e], ..].  Every element
 *   of out is written (an empty row gives 0), nothing is added atomically, and the result does not depend on the run.
 *   The table must come from axis_table with n = the length of `axis` (pull: n_out = m; transposed: the table's m is
 *   the length of `axis` and n_out its n): col is not checked on the device. */
size_t bfm_spline_axis_table_workspace(int m, int n, int order);
int bfm_spline_axis_table(const float* coord, int m, int n, int order, int bound, int extrapolate, int ties_even,
                          int transpose, int32_t* rowptr, int32_t* col, float* val, void* workspace,
                          size_t workspace_bytes, bfm_stream_t stream);
int bfm_spline_axis_pass(const float* in, int64_t lead, int nx, int ny, int nz, int axis, const int32_t* rowptr,
                         const int32_t* col, const float* val, int n_out, float* out, bfm_stream_t stream);
/* interpol.grid_pull on an integer image, the label branch of utils/interpol/api.py:182-193: the reference pulls the
 * indicator of every label of unique() and keeps per output voxel the label with the largest interpolated weight.  Here
 * in one pass over the output: w_L = the sum over the taps of the voxel's footprint that hold L of weight * bound sign
 * (nodes, signs, weights, mask and argument checks of the _spline exports above; fp32, fixed tap order), out = the label
 * with the largest w_L > 0, the smallest label among equal sums (the reference walks the labels in ascending order and
 * replaces on a strict >), 0 where no sum is positive (outside the field of view without extrapolation, outside a `zero`
 * bound, a footprint of negative `dst1` / `dst2` taps).  The cost does not depend on the number of labels.
 * inp (Bi,C,nx,ny,nz) and out (max(Bi,Bg),C,ox,oy,oz) have the element type `dtype`; grid (Bg,ox,oy,oz,3) fp32.
 * variant: how the thread keeps its (label, sum) table -- AUTO: REGS for the all-nearest / all-linear footprints (1 / 8
 * taps), PASSES otherwise; LDS (a per-thread LDS slice), REGS (the footprint in registers, rescanned per tap) and PASSES
 * (four register slots, the footprint walked again while labels are left) force one for every order (measurements).
 * All give the same bits. */
#define BFM_LABEL_U8 0
#define BFM_LABEL_I16 1
#define BFM_LABEL_I32 2
#define BFM_LABEL_I64 3
#define BFM_LABEL_PULL_AUTO 0
#define BFM_LABEL_PULL_LDS 1
#define BFM_LABEL_PULL_REGS 2
#define BFM_LABEL_PULL_PASSES 3
int bfm_label_pull3d(const void* inp, int dtype, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                     int oy, int oz, const int* bound, const int* order, int extrapolate, int variant, void* out,
                     bfm_stream_t stream);
/* interpol.identity_grid / affine_grid / add_identity_grid_ in 3-D -- utils/interpol/api.py:455-560.
 * affine_grid3d: out (nb,nx,ny,nz,3), out[b,x,y,z,r] = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3] with m =
 *   mat[b] (nb,3,4 row-major, device), the summation order of the reference's matvec(lin, idx) + off, every product and
 *   sum rounded on its own; mat NULL: the identity grid (x, y, z).  add_identity_grid3d: disp (nb,nx,ny,nz,3) += (x, y, z)
 *   in place.  is_f64 0: fp32, otherwise fp64.  Bit-equal to the reference in both. */
int bfm_affine_grid3d(const void* mat, int is_f64, int64_t nb, int nx, int ny, int nz, void* out, bfm_stream_t stream);
int bfm_add_identity_grid3d(void* disp, int is_f64, int64_t nb, int nx, int ny, int nz, bfm_stream_t stream);
/* Resampling through a voxel-to-voxel matrix (brainfm_amd/native.py, csrc/affine_pull.hip; no counterpart in the
 * reference, whose results stay on the processed grid of prepare_image, utils/test_utils.py:235-284).  M_host: 12 HOST
 * doubles, row-major 3 x 4, destination index (i,j,k) -> source coordinate, evaluated in fp64 on the device as
 * ((M[r][0]*i + M[r][1]*j) + M[r][2]*k) + M[r][3] with every operation rounded on its own.
 * affine_pull_multi: out [K][X][Y][Z] fp32 <- K fp32 maps of (D,H,W), map m at src + m * map_stride (elements, >= D*H*W:
 *   the stitched buffer of the tile flows is read in place).  mode_host[m] 0: trilinear, f = floor(x), wc = (float)(x - f),
 *   wf = 1.f - wc, corners f and f + 1, a corner outside the source counts as 0 (grid_sample's padding_mode='zeros',
 *   align_corners=True), summed in the c00 .. c chain of Generator/utils.py:177-185; 1: nearest, index floor(x + 0.5),
 *   the 4-byte pattern copied, 0 outside.  All offsets are 64-bit.
 * affine_pull_argmax: label [X][Y][Z] int32 <- post (D,H,W,C) fp32 channels-last, the layout the network tail leaves the
 *   posteriors in.  Every channel is interpolated by the linear rule above; label = lut[c*], c* the first channel whose
 *   value is > 0 and > every earlier channel's (ties: the lower channel; a NaN never wins); 0 where no value is positive,
 *   which covers everything outside the field of view.  best (may be NULL): the winning value, 0 where there is none.
 *   No posterior volume on the destination grid is written.
 * affine_pull_route (host arithmetic, no device needed; the launcher asks here too): the lanes that share one voxel in
 *   affine_pull_argmax when it is called with lanes = 0: the smallest power of two at which a lane takes at most five
 *   channels, at most 16 (the widths were timed at C = 18 and 56, profiles/native.txt).  < 0: BFM_E_ARG.
 *   lanes = 1, 2, 4 .. 64 forces a width (1: one thread per voxel looping over the channels); every width gives the same
 *   bits, scripts/bench_native.py times them side by side. */
int bfm_affine_pull_multi(const float* src, int64_t map_stride, int K, int D, int H, int W, const double* M_host,
                          const int* mode_host, int X, int Y, int Z, float* out, bfm_stream_t stream);
int bfm_affine_pull_argmax(const float* post, int C, int D, int H, int W, const int32_t* lut, const double* M_host, int X,
                           int Y, int Z, int lanes, int32_t* label, float* best, bfm_stream_t stream);
int bfm_affine_pull_route(int C);
/* BaseGen.deform_grid -- Generator/datasets.py:264-303: (xc+F) -> A*. + c2, clamp to the source shape, and the
 * six global min/max (minmax = {min x,y,z, max x,y,z}, device).  F is [n][3] or NULL. */
size_t bfm_deform_grid_workspace(int sx, int sy, int sz);
int bfm_deform_grid(const float* F, int sx, int sy, int sz, const float* A_host /*[9]*/, const float* c2_host /*[3]*/,
                    const int* shp_host /*[3]*/, float* xx, float* yy, float* zz, float* minmax /*[6]*/,
                    void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* generate_sample core -- Generator/datasets.py:366-372: mus[round(G)] + sigmas[round(G)]*randn, clamp >= 0
 * (label 77 merged into 2). */
/* generate_sample's pathology branch -- Generator/datasets.py:388-396: cerebral[i] = (round(G[i]) == 0) ? 0 : syn[i]
 * (G == 77 counts as 2, :368) and the four sums behind wm_mean / gm_mean: stats[0..3] = sum(syn | label in {2,41}),
 * count of those, sum(syn | label not in {0,2,41}), count (fp64, written whole).  partials: workspace of
 * 4 * BFM_CLASS_STATS_BLOCKS doubles -- the blocks' sums, added in block order, so the result does not depend on the
 * run (the reference's torch sums are deterministic on CPU; pathol_direction = gm_mean > wm_mean hangs on them). */
#define BFM_CLASS_STATS_BLOCKS 1024
int bfm_label_class_stats(const float* G, const float* syn, int64_t n, float* cerebral, double* stats /*[4]*/,
                          double* partials, bfm_stream_t stream);
int bfm_label_gauss(const float* G, const float* mus, const float* sigmas, const float* randn, int64_t n, int ntab,
                    float* out, bfm_stream_t stream);
/* onehotmatrix[lut[S]] -- Generator/utils.py:408-411: out [n][n_labels]. */
int bfm_onehot_lut(const int32_t* S, const int32_t* lut, int nlut, int n_labels, int64_t n, float* out,
                   bfm_stream_t stream);

/* Perlin noise on a lattice of host-drawn gradients -- ShapeID/perlin3d.py:38-83 (fp64, NumPy semantics).
 * grad: [(rx+1)(ry+1)(rz+1)][3]. */
int bfm_perlin3d(const double* grad, int sx, int sy, int sz, int rx, int ry, int rz, double* out, bfm_stream_t stream);
/* np.percentile support (perlin3d.py:84-90): 16-bit digit histogram of the order-preserving key of each
 * double among keys whose higher bits equal `prefix`; four passes select an order statistic. */
int bfm_radix_hist_f64(const double* x, int64_t n, uint64_t prefix, int shift, uint32_t* hist65536, bfm_stream_t stream);
int bfm_threshold_mask_f64(const double* x, int64_t n, double thr, double* masked, double* mask, bfm_stream_t stream);
/* stream_3D(gradient_c(a), gradient_c(b), gradient_c(c)) * mult -- ShapeID/misc.py:66-80,198-259. */
int bfm_curl3d(const double* a, const double* b, const double* c, int sx, int sy, int sz, float mult, float* Vx,
               float* Vy, float* Vz, bfm_stream_t stream);
/* AdvDiffPDE.forward, perf_pattern='adv', V_type='vector_div_free' -- ShapeID/DiffEqs/pde.py:616-640:
 * out = -(Vx*dxC + Vy*dyC + Vz*dzC) with upwind differences of the (optionally Neumann-conditioned) field. */
int bfm_advect_upwind_rhs(const void* C, int c_is_f64, const float* Vx, const float* Vy, const float* Vz, int sx,
                          int sy, int sz, int neumann_bc, float* out, bfm_stream_t stream);
/* Runge-Kutta tensor arithmetic of Dopri5Solver (ShapeID/DiffEqs/rk_common.py:22-61, misc.py:22-25,84-170,
 * interp.py:5-65).  k[j] are fp32 stage derivatives, coef[j] the fp32 value of (dt*c_j). */
typedef struct { const float* k[7]; float coef[7]; int nk; } bfm_kset_t;
int bfm_rk_combine(const void* y0 /*NULL: out = sum*/, int is_f64, const bfm_kset_t* ks, void* out, int64_t n,
                   bfm_stream_t stream);
size_t bfm_reduce_workspace(void);
int bfm_rk_error_sumsq(const bfm_kset_t* ks, const void* y0, const void* y1, int is_f64, double atol, double rtol,
                       int64_t n, double* out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_scaled_sumsq(const void* a, const void* b /*may be NULL*/, int ab_is_f64, const void* y0, int y_is_f64,
                     double atol, double rtol, int64_t n, double* out, void* workspace, size_t workspace_bytes,
                     bfm_stream_t stream);
int bfm_dopri5_dense_eval(const void* y0, const void* y1, int is_f64, const bfm_kset_t* mid, double dt, double x,
                          void* out, int64_t n, bfm_stream_t stream);
/* op: 0 min, 1 max, 2 sum(x), 3 sum(x*y); result in fp64 (deterministic two-stage reduction). */
int bfm_reduce_f32(int op, const float* x, const float* y, int64_t n, double* out, void* workspace,
                   size_t workspace_bytes, bfm_stream_t stream);
int bfm_reduce_f64(int op, const double* x, const double* y, int64_t n, double* out, void* workspace,
                   size_t workspace_bytes, bfm_stream_t stream);

/* ---- the generator item without host round trips (round 4; brainfm_amd/csrc/synth_item.hip) --------------------------
 * BrainIDGen.__getitem__ (Generator/datasets.py:700-757) re-reads every NIfTI volume of the case and crops it on the
 * host per item (Generator/utils.py:296-305); here the case's volumes stay resident in HBM, the crop is a box inside
 * them, scalar operands (min / max / sums / order statistics) stay in device memory between kernels, and short chains
 * between two reductions are one kernel.  The arithmetic and its order are those of the unfused entry points above. */

/* torch.randn(shape, device) of the generator: Philox4x32-10 counter (element index / 4, offset) under `seed`,
 * Box-Muller, out = scale * N(0,1).  A different stream from torch's (RNG-stream parity across devices is not a goal
 * of the reference either); the same (seed, offset) gives the same field on every run and device. */
int bfm_randn_philox(float* out, int64_t n, uint64_t seed, uint64_t offset, float scale, bfm_stream_t stream);

/* BaseGen.generate_deformation / deform_grid (datasets.py:187-303) with myzoom_torch(Fsmall, size / small)
 * (utils.py:200-257) folded in: the zoomed field is evaluated per voxel from Fsmall [fnx][fny][fnz][3] and the zoom
 * tables instead of being written and read back (Fsmall NULL: affine only).  _minmax writes the six extrema of the
 * clamped coordinates (device, {min x,y,z, max x,y,z}) and nothing else; the host reads them (the reference
 * synchronises there too, datasets.py:296-301), and _write stores the coordinates minus lo (+ F [n][3] on request).
 * photo_zero_y: F[..., 1] = 0 (photo mode, datasets.py:243). */
size_t bfm_deform_zoom_workspace(void);
int bfm_deform_zoom_minmax(const float* Fsmall, int fnx, int fny, int fnz, const bfm_zoom_axis_t* ax, int photo_zero_y,
                           int sx, int sy, int sz, const float* A_host, const float* c2_host, const int* shp_host,
                           float* minmax6, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_deform_zoom_write(const float* Fsmall, int fnx, int fny, int fnz, const bfm_zoom_axis_t* ax, int photo_zero_y,
                          int sx, int sy, int sz, const float* A_host, const float* c2_host, const int* shp_host,
                          const float* lo_host /*[3]*/, float* xx, float* yy, float* zz, float* F_out /*or NULL*/,
                          bfm_stream_t stream);

/* The surface task.  BaseGen.random_nonlinear_transform with 'surface' in the tasks -- Generator/datasets.py:214-224:
 *     s = 1 / 2**n; Fsvf = F * s; n times: Fsvf += fast_3D_interp_torch(Fsvf, xx + Fsvf[...,0], yy + Fsvf[...,1],
 *     zz + Fsvf[...,2], 'linear'); the same from Fsvf_neg = -F * s.
 * F, F_out, Fneg_out: [sx][sy][sz][3] fp32 (device, distinct).  One launch per step covers both directions; the first step
 * reads F and applies +-s itself; each step reads one buffer and writes another (the interpolation is complete before the
 * add), one scratch buffer per direction in the workspace (>= bfm_svf_integrate_workspace; none needed for n <= 1), and
 * the start buffer is chosen by the parity of n so that the last step writes F_out / Fneg_out.  n_steps = 0: F * 1 and
 * -F * 1.  Each voxel's arithmetic is fast_3D_interp_torch's in its order: bit-identical to the reference's CPU path. */
size_t bfm_svf_integrate_workspace(int sx, int sy, int sz);
int bfm_svf_integrate(const float* F, int sx, int sy, int sz, int n_steps, float* F_out, float* Fneg_out, void* workspace,
                      size_t workspace_bytes, bfm_stream_t stream);
/* read_and_deform_surface -- Generator/utils.py:479-531, the vertex arithmetic of up to BFM_VERTEX_SETS_MAX sets in one
 * launch, in place on V [n][3] fp32 (device):  V -= c2; V = V @ Ainv.T; V += fast_3D_interp_torch(Fneg, V[:,0] + c2[0],
 * V[:,1] + c2[1], V[:,2] + c2[2]) (0 where not ok); V += c2; flip: V[:,0] = size0 - 1 - V[:,0].  Fneg [sx][sy][sz][3]
 * (device); Ainv_host = inverse(A), row-major [9], c2_host [3].  Faces are not touched (the host swaps left / right). */
#define BFM_VERTEX_SETS_MAX 4
typedef struct {
    float* V;
    int64_t n;
} bfm_vertex_set_t;
int bfm_deform_vertices(const float* Fneg, int sx, int sy, int sz, const bfm_vertex_set_t* sets, int n_sets,
                        const float* Ainv_host, const float* c2_host, int flip, int size0, bfm_stream_t stream);

/* read_and_deform and its callers (Generator/utils.py:296-322; _image :331-345, _distance :376-400,
 * _registration :462-473) for up to BFM_GATHER_MAX_JOBS volumes that share one coordinate field, straight from the
 * resident full volumes [nx][ny][nz]: box6 = {x1,y1,z1,x2,y2,z2} is the crop the reference takes (upper ends clipped
 * to the volume like a NumPy slice); validity and corner clamps of fast_3D_interp_torch are evaluated in CROP space.
 * Per job: texel -> pre (0 none, 1 nan_to_num, 2 nan_to_num then (x - mean) / scale) -> trilinear; invalid
 * coordinates take 0 or, with default_max, the crop's maximum after `pre` (read_and_deform's default_value_linear);
 * then r / post_div (0 = off), clamp, r * sign (0 = off), written at the voxel (mirrored along axis 0 with flip0).
 * want_minmax leaves min / max of the job's output in scalars[BFM_GATHER_MAX_JOBS + 2j (+1)]; scalars[j] holds the
 * default value of job j.  scalars: 3 * BFM_GATHER_MAX_JOBS doubles (device). */
#define BFM_GATHER_MAX_JOBS 12
typedef struct {
    const float* src; float* out;
    float mean, scale; int pre; int default_max;
    float post_div; int clamp; float clamp_lo, clamp_hi; float sign; int want_minmax;
} bfm_gather_job_t;
size_t bfm_gather_targets_workspace(void);
int bfm_gather_targets(const bfm_gather_job_t* jobs, int njobs, int nx, int ny, int nz, const int* box6_host,
                       const float* II, const float* JJ, const float* KK, int sx, int sy, int sz, int flip0,
                       double* scalars, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* I -= min(I); I /= max(I) (read_and_deform_image, utils.py:340-342) with {min, max} of I in device memory. */
int bfm_minmax_normalise(float* x, int64_t n, const double* minmax_dev, bfm_stream_t stream);
/* read_and_deform_segmentation (utils.py:402-425): nearest gather from the resident int32 label volume (crop-space
 * rounding and clamps), lut, one-hot rows out [sx][sy][sz][n_labels]; flip0: torch.flip(., [0])[..., vflip]. */
int bfm_gather_onehot(const int32_t* S, int nx, int ny, int nz, const int* box6_host, const float* II, const float* JJ,
                      const float* KK, int sx, int sy, int sz, int flip0, const int32_t* lut, int nlut, int n_labels,
                      const int32_t* vflip /*[n_labels] or NULL*/, float* out, bfm_stream_t stream);
/* the same, out as [n_labels][sx][sy][sz]: the element order the reference's .permute([3, 0, 1, 2]) view is read in
 * (Generator/utils.py:423-425), so that no consumer has to make it contiguous */
int bfm_gather_onehot_rows(const int32_t* S, int nx, int ny, int nz, const int* box6_host, const float* II, const float* JJ,
                      const float* KK, int sx, int sy, int sz, int flip0, const int32_t* lut, int nlut, int n_labels,
                      const int32_t* vflip /*[n_labels] or NULL*/, float* out, bfm_stream_t stream);

/* np.percentile(x, q) (method 'linear', ShapeID/perlin3d.py:84-90) without leaving the device: radix select of the
 * order statistic k_lo (six passes over 11 / 9-bit digits of the order-preserving key, block histograms in LDS), the
 * next one where needed, NumPy's _lerp with weight t.  out3 (device) = {percentile, x_(k_lo), x_(k_lo+1)}. */
size_t bfm_percentile_workspace(void);
int bfm_percentile_f64(const double* x, int64_t n, int64_t k_lo, int need_next, double t, double* out3, void* workspace,
                       size_t workspace_bytes, bfm_stream_t stream);
/* generate_perlin_noise_3d's mask (perlin3d.py:86-90) with the threshold in device memory: masked = x * (x >= thr),
 * mask (optional) = (x >= thr); max_out = max(masked).  binarize (Generator/utils.py:65-72): P = (p >= thres * max)
 * in p's dtype, sum_out = sum(P). */
size_t bfm_shape_workspace(void);
int bfm_shape_threshold_f64(const double* noise, int64_t n, const double* thr_dev, double* masked, double* mask,
                            double* max_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_shape_binarize(const void* p, int is_f64, int64_t n, const double* max_dev, double thres, void* P,
                       double* sum_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* generate_sample's pathology branch (datasets.py:398-399): target['pathology'][cer == 0] = 0 and the same for
 * pathology_prob, in place in their own dtype; sum_out = sum of the masked pathology (the test of :322 / :387). */
int bfm_pathology_mask(void* P, void* Pprob, int is_f64, const float* cerebral, int64_t n, double* sum_out,
                       void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* encode_pathology (datasets.py:496-518) with I_mu = sum(I*P) / sum(P) kept on the device (dotsum_out[2]); u4 = the
 * uniform draws behind pth_mus[0], pth_mus[1], pth_sigmas[0], pth_sigmas[1]; direction 1 / 0, or -1 to take
 * gm_mean > wm_mean from bfm_label_class_stats' sums (datasets.py:392-404) without reading them back. */
size_t bfm_pathology_encode_workspace(void);
int bfm_pathology_encode_dev(const float* I, const void* P, const void* Pprob, int is_f64, const float* randn,
                             const float* u4_host, int direction, const double* class_stats_dev, int64_t n, float* out,
                             double* dotsum_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* resample_resolution's sample (utils.py:600-606): fast_3D_interp_torch on meshgrid(ax, ay, az), the grid never
 * materialised. */
int bfm_interp3d_linear_axes(const float* X, int nx, int ny, int nz, const float* ax, const float* ay, const float* az,
                             int ox, int oy, int oz, float default_value, float* out, bfm_stream_t stream);
/* augment_sample's tail (datasets.py:340-352): input = I / max, residual = high_res / max - input (optional), both
 * mirrored along axis 0 with flip0; max in device memory. */
int bfm_sample_finalize(const float* I, const float* high_res, int sx, int sy, int sz, const double* max_dev, int flip0,
                        float* input_out, float* residual_out, bfm_stream_t stream);

/* Dormand-Prince integration of AdvDiffPDE ('adv', div-free V) with the step controller on the device
 * (ShapeID/DiffEqs/dopri5.py:58-172, rk_common.py:22-61, misc.py:145-170, interp.py:5-65, pde.py:616-640): one kernel per
 * stage (stage state evaluated at the stencil points from y and the k_j, never stored), error norm, accept / reject with
 * the reference's forced-accept clamps, next step size and the dense outputs at t_out all computed from / into `state`
 * (device, bfm_dopri5_advect_state_bytes()).  The host calls _init, copies y0 into y[0] and sol[0], f(t0, y0) into f[0],
 * then enqueues steps in chunks with _steps and reads the state block back between chunks: its int fields at byte offset
 * 40 are {cur, done, next_out, nsteps, naccept, accepted, err}; steps enqueued past the end do nothing.  y / sol are in
 * the state dtype (fp64 or fp32), stages fp32.  workspace: bfm_dopri5_advect_workspace(sx, sy, sz) bytes. */
typedef struct {
    void* y[2]; float* f[2]; float* k[5];
    const float *Vx, *Vy, *Vz;
    int sx, sy, sz, neumann_bc, is_f64;
    double atol, rtol, tol_min_dt, dt_max, safety, ifactor, dfactor;
    const double* t_out /*device [nt]*/; int nt; void* sol /*[nt][n]*/;
    void* state; void* workspace;
} bfm_dopri5_advect_t;
size_t bfm_dopri5_advect_state_bytes(void);
size_t bfm_dopri5_advect_workspace(int sx, int sy, int sz);
int bfm_dopri5_advect_init(const bfm_dopri5_advect_t* d, double t0, double dt0, bfm_stream_t stream);
int bfm_dopri5_advect_steps(const bfm_dopri5_advect_t* d, int nsteps, bfm_stream_t stream);

/* Fixed-grid integration of the same PDE: euler, midpoint and rk4, the 3/8 rule (ShapeID/DiffEqs/fixed_grid.py:5-33,
 * solvers.py:158-207 FixedGridODESolver.integrate, rk_common.py:72-78 rk4_alt_step_func; RHS pde.py:616-640).  The grid is
 * the requested times, so step i reads row i of sol and writes row i + 1; the call enqueues all nt - 1 steps (1, 2 or 4
 * kernels each) and reads nothing back.  On entry row 0 of sol holds y0.  A stage kernel forms the stage state
 * y + sum_j c_j k_j (bfm_rk_combine's expression) with the Neumann replicate on an LDS box with its halo and the upwind
 * RHS from it; the last stage of a step adds bfm_rk_combine's final sum and stores y1 instead of its k.
 * coef: HOST array of (nt - 1) x bfm_ode_fixed_ncoef(method) fp32 values, per step the coefficients bfm_rk_combine
 * would be given, (dt * c) in the state dtype rounded to fp32:
 *   euler     {dt}                                      y1 = y + dt k1
 *   midpoint  {dt/2, dt}                                k2 = f(y + dt/2 k1);  y1 = y + dt k2
 *   rk4       {dt/3, -dt/3, dt, dt, -dt, dt, dt/8, 3dt/8, 3dt/8, dt/8}
 *             k2 = f(y + dt/3 k1); k3 = f(y - dt/3 k1 + dt k2); k4 = f(y + dt k1 - dt k2 + dt k3); y1 = y + sum
 * k: fp32 stage buffers of n voxels (euler 0, midpoint 1, rk4 3).  sx, sy, sz >= 3. */
enum { BFM_ODE_EULER = 0, BFM_ODE_MIDPOINT = 1, BFM_ODE_RK4 = 2 };
typedef struct {
    void* sol /*[nt][n], state dtype*/; float* k[3];
    const float *Vx, *Vy, *Vz;
    int sx, sy, sz, neumann_bc, is_f64, method, nt;
    const float* coef /*host*/;
} bfm_ode_fixed_advect_t;
int bfm_ode_fixed_ncoef(int method);
int bfm_ode_fixed_advect(const bfm_ode_fixed_advect_t* d, bfm_stream_t stream);

/* The other configurations of AdvDiffPDE (ShapeID/DiffEqs/pde.py:331-640, 3-D, unit spacing, batch of one): the diffusion
 * terms Grad_constantD / Grad_scalarD / Grad_diagD / Grad_fullD (:362-441), the general velocity Grad_vectorV (:511-524)
 * and their sum out_V + out_D (:623-639).  A terms block goes beside the structs above, whose layout is unchanged; NULL
 * terms is the generator's configuration ('adv', divergence-free V), and the calls above are that case.
 *   perf       BFM_PDE_ADV, BFM_PDE_DIFF or both ('adv', 'diff', 'adv_diff'); without ADV the V pointers may be NULL
 *   d_type     BFM_PDE_D_* (with DIFF); the 'full_*' names of Grad_Ds are BFM_PDE_D_FULL
 *   v_general  0: Grad_div_free_vectorV;  1: Grad_vectorV, the upwind term minus C * divV (promoting an fp64 state's
 *              value to fp64 before it is rounded to the fp32 stage)
 *   D          fp32 fields of n voxels: {D} (scalar), {Dxx, Dyy, Dzz} (diag), {Dxx, Dyy, Dzz, Dxy, Dyz, Dxz} (full)
 *   G          the time-invariant factors of c_x C, c_y C, c_z C, by bfm_pde_central_sum: scalar {c_x D, c_y D, c_z D},
 *              diag {c_x Dxx, c_y Dyy, c_z Dzz}, full the row sums {c_x Dxx + c_y Dxy + c_z Dxz, c_x Dxy + c_y Dyy +
 *              c_z Dyz, c_x Dxz + c_y Dyz + c_z Dzz} (:435-437)
 *   divV       c_x Vx + c_y Vy + c_z Vz (:517-524), with v_general
 * f / b / c: gradient_f / gradient_b / gradient_c (:13-186).  The stage kernels are those of the calls above with the
 * right-hand side chosen at compile time; sx, sy, sz >= 3. */
enum { BFM_PDE_ADV = 1, BFM_PDE_DIFF = 2 };
enum { BFM_PDE_D_CONSTANT = 1, BFM_PDE_D_SCALAR = 2, BFM_PDE_D_DIAG = 3, BFM_PDE_D_FULL = 4 };
typedef struct {
    int perf, d_type, v_general; float D_const;
    const float* D[6]; const float* G[3]; const float* divV;
} bfm_pde_terms_t;
/* out = sum_j c_{axis[j]}(f[j]), j < nterms <= 3, added left to right in fp32 -- gradient_c, pde.py:127-186 (the derived
 * fields G and divV above).  f, axis: host arrays of device pointers / axis numbers 0..2. */
int bfm_pde_central_sum(const float* const* f, const int* axis, int nterms, int sx, int sy, int sz, float* out,
                        bfm_stream_t stream);
/* AdvDiffPDE.forward for any built configuration -- pde.py:616-640.  out is fp32, or fp64 (out_is_f64) for v_general
 * with an fp64 C, the one case where the reference's result is fp64. */
int bfm_advdiff_rhs(const void* C, int c_is_f64, const float* Vx, const float* Vy, const float* Vz,
                    const bfm_pde_terms_t* terms, int sx, int sy, int sz, int neumann_bc, void* out, int out_is_f64,
                    bfm_stream_t stream);
/* bfm_dopri5_advect_init / _steps and bfm_ode_fixed_advect with a terms block -- dopri5.py:58-172, fixed_grid.py:5-33 over
 * pde.py:616-640. */
int bfm_dopri5_advdiff_init(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* terms, double t0, double dt0,
                            bfm_stream_t stream);
int bfm_dopri5_advdiff_steps(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* terms, int nsteps, bfm_stream_t stream);
int bfm_ode_fixed_advdiff(const bfm_ode_fixed_advect_t* d, const bfm_pde_terms_t* terms, bfm_stream_t stream);

/* ---- backward pass of the SingleConv block and its neighbours (first correct version) -------------------
 * The reference trains through torch autograd over buildingblocks.py:31-60 (GroupNorm -> Conv3d -> LeakyReLU),
 * :185-186 (MaxPool3d(2)), :265-276,361-363 (nearest upsample + concat).
 *   lrelu_bwd    dP = dY * (Y > 0 ? 1 : slope)                 (n % 4 == 0)
 *   wgrad        dW[co][ci][27] = sum_v dP[v][co] * GN(x)[v+tap][ci]   (exact fp32 matrix cores, fixed split order)
 *   data grad    = bfm_conv3x3x3_mfma / _direct on the transposed, tap-mirrored weights with identity affine, slope 1
 *   gn_bwd       dXn -> dA (skip channels), dB (low-res channels: sum over the replica box), dgamma, dbeta
 *   maxpool2_bwd gradient to the first maximum of each 2x2x2 window (scan order dz,dy,dx), zeros elsewhere */
int bfm_lrelu_bwd(const float* dY, const float* Y, int64_t n, float slope, float* dP, bfm_stream_t stream);
/* the same, also writing max |dP| (device float; the split-fp16 weight / data gradient kernels scale dP by it) */
int bfm_lrelu_bwd_ex(const float* dY, const float* Y, int64_t n, float slope, float* dP, float* absmax,
                     bfm_stream_t stream);
/* Workspace bytes of bfm_conv3x3x3_wgrad / _ex for a layer of Cin = CA + CB input channels: an upper bound over the routes
 * below and over every way to divide Cin into skip and upsampled channels.  bfm_conv3x3x3_wgrad_plan gives the exact need
 * of one layer; _ex still asks for this bound (BFM_E_WORKSPACE below it). */
size_t bfm_conv3x3x3_wgrad_workspace(int Cin, int Cout, int D, int H, int W);
/* The route bfm_conv3x3x3_wgrad_ex takes for a layer (CA skip / plain channels, CB channels upsampled from (d, h, w); d, h, w
 * are not read when CB == 0), from the layer alone: no device call.  allow: bit 0 the wave-specialised kernel may be used,
 * bit 1 an exact 2x join may run folded; negative: what _ex uses in this process (BFM_WGRAD_WS, BFM_WGRAD_UPFOLD and the
 * device's LDS limit, asked once).  plan_out [20]:
 *   [0] route  0 wave-specialised kernel on a plain layer (passes 3, Cout % 64, CA % 32 == 0, CB == 0, bit 0)
 *              1 folded join (passes 3, bit 1, CB % 32 == 0, (D, H, W) == 2 (d, h, w), h >= 4, w >= 16): launch 0 runs the skip
 *                channels, launch 1 the upsampled channels on the low-res tensor
 *              2 f16 tiles on all channels (passes 3, Cout % 64, Cin % 32, CA % 32 == 0)
 *              3 fp32 tiles (the same widths at passes 0)          4 fp32 columns (every other width)
 *   [1]        route 1: 1 when the skip channels run on the wave-specialised kernel (bit 0), 0 on f16 tiles
 *   [2..10]    launch 0: tile grid nbz, nby, nbx, tiles (route 4: the D x H rows), workgroup columns, S, per, then byte offset
 *              and size of its partials in the workspace.  The launch runs S x columns workgroups; each takes `per`
 *              tiles, the last maybe fewer, none is empty.  One rule for every tiled kernel: S = ceil(tiles / per) with
 *              per = ceil(tiles / min(tiles, max(1, 512 / columns))); route 4 splits rows under ceil(2048 / columns).
 *   [11..19]   launch 1 of route 1, the same nine; zeros on the other routes
 * *exact_bytes_out (may be NULL): the end of the last region, <= bfm_conv3x3x3_wgrad_workspace(CA + CB, Cout, D, H, W). */
int bfm_conv3x3x3_wgrad_plan(int CA, int CB, int Cout, int D, int H, int W, int d, int h, int w, int passes, int allow,
                             int64_t* plan_out /*[20]*/, size_t* exact_bytes_out);
/* The whole backward of the first SingleConv of a conditioned network (GroupNorm(1, Cin) + Conv3d(Cin, Cout, 3) on the
 * network's input; torch autograd over buildingblocks.py:31-60 for the model of Trainer/models/__init__.py:423-437) as ONE
 * correlation on the exact-fp32 matrix core.  The input is data, so no input gradient is formed: over the raw input x,
 *   Q[o,c,t] = sum_v dP[v,o] x[v+t,c],  S[o,t] = sum_v dP[v,o]   (v+t inside the volume)
 *   dW[o,c,t] = scale_c Q + shift_c S,  dgamma_c = rstd sum_{o,t} W (Q - mean S),  dbeta_c = sum_{o,t} W S.
 * dP [D][H][W][Cout] (after lrelu_bwd, 16-byte aligned), x channels-last [D][H][W][Cin], w_raw [Cout][Cin][27], scale /
 * shift [Cin] and mean / rstd [1] as bfm_gn_stats_train wrote them (one group).  Cin in {2,3,4}, Cout in {32,64}, any
 * D,H,W >= 1 with D*H*W < 2^31; BFM_E_SHAPE otherwise, nothing launched.  Per-workgroup fp32 partials folded in fp64 in a
 * fixed order, no atomics: the same bits on every run.  workspace: bfm_stem_mc_bwd_workspace() bytes, 8-byte aligned. */
size_t bfm_stem_mc_bwd_workspace(int Cin, int Cout, int D, int H, int W);
int bfm_stem_mc_bwd(const float* dP, int Cout, const float* x, int Cin, int D, int H, int W, const float* w_raw,
                    const float* scale, const float* shift, const float* mean, const float* rstd,
                    float* dW /*[Cout][Cin][27]*/, float* dgamma /*[Cin]*/, float* dbeta /*[Cin]*/, void* workspace,
                    size_t workspace_bytes, bfm_stream_t stream);
/* The input gradient of the same layer (GroupNorm(1, Cin) + Conv3d(Cin, Cout, 3, padding=1)) with respect to ONE input
 * channel, optionally chained through the masking of the two-stage model into the stage-0 logit (torch autograd over
 * buildingblocks.py:31-60 and Trainer/engine.py:238, input_masked = input * (1 - sigmoid(raw0)), in
 * train_one_epoch_twostage, engine.py:193-318).  With xhat = (x_cl - mean) rstd and N = Cin D H W:
 *   G_c[u]  = sum_{o,k} dP[u - k + 1, o] W[o, c, k]                        (zero outside the volume; c = channel)
 *   dX_c[u] = rstd (gamma_c G_c[u] - m1 - xhat_c[u] m2),  m1 = sum gamma dbeta / N,  m2 = sum gamma dgamma / N
 *   dRaw[col_offset + u voxel_stride] += -x_raw[u] dX_c[u] p[u] (1 - p[u])
 * dgamma / dbeta [Cin]: what the layer's parameter backward (bfm_stem_mc_bwd or bfm_gn_bwd) produced for the same dP.
 * Only channel c's G is formed (exact-fp32 matrix core), in one launch.  dx [D][H][W] (may be NULL) receives dX_c; x_raw
 * and p (both NULL: no chain) are the unmasked image and sigmoid(raw0); dRaw is added to, one writer per voxel, no
 * atomics: the same bits on every run.  Shapes as bfm_stem_mc_bwd, 0 <= channel < Cin: BFM_E_SHAPE otherwise; a NULL
 * mandatory pointer (or neither dx nor the chain asked for): BFM_E_ARG; nothing is launched or written on error.
 * dP 16-byte aligned. */
int bfm_stem_mc_dgrad(const float* dP, int Cout, const float* x_cl, int Cin, int D, int H, int W, const float* w_raw,
                      const float* gamma, const float* mean, const float* rstd, const float* dgamma, const float* dbeta,
                      int channel, float* dx /*[D][H][W] or NULL*/, const float* x_raw, const float* p, float* dRaw,
                      int64_t col_offset, int64_t voxel_stride, bfm_stream_t stream);
/* The chain alone, for an input gradient that already exists (bfm_gn_bwd's dA, read with a stride):
 * dRaw[col_offset + u voxel_stride] += -x_raw[u] dx[u dx_stride] p[u] (1 - p[u]), u < n.  The same expression, and the
 * same bits, as bfm_stem_mc_dgrad's epilogue (Trainer/engine.py:238 under autograd). */
int bfm_mask_chain_bwd(const float* dx, int64_t dx_stride, const float* x_raw, const float* p, int64_t n, float* dRaw,
                       int64_t col_offset, int64_t voxel_stride, bfm_stream_t stream);
int bfm_conv3x3x3_wgrad(const float* dP, int Cout, const float* A, int CA, const float* B, int CB, int D, int H, int W,
                        const bfm_upsample_t* up, const float* scale, const float* shift, float* dW /*[Cout][Cin][27]*/,
                        void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* passes = 0: exact fp32 matrix core (= bfm_conv3x3x3_wgrad).  passes = 3: split-fp16 (hi*hi + hi*lo + lo*hi, fp32
 * accumulate -- the forward kernels' accuracy class) on layers with Cout % 64 == 0, CA % 32 == 0, Cin % 32 == 0, the fp32
 * kernel elsewhere; needs dp_bound [1] = max |dP| and x_bound [G] = max |GroupNorm-applied input| per group (device). */
int bfm_conv3x3x3_wgrad_ex(const float* dP, int Cout, const float* A, int CA, const float* B, int CB, int D, int H, int W,
                           const bfm_upsample_t* up, const float* scale, const float* shift, const float* dp_bound,
                           const float* x_bound, int G, int passes, float* dW, void* workspace, size_t workspace_bytes,
                           bfm_stream_t stream);
size_t bfm_gn_bwd_workspace(int C, int D, int H, int W);
int bfm_gn_bwd(const float* dXn, const float* A, int CA, const float* B, int CB, int D, int H, int W,
               const bfm_upsample_t* up, const int32_t* startD, const int32_t* startH, const int32_t* startW,
               const float* mean, const float* rstd, const float* gamma, int G, float* dA, float* dB, float* dgamma,
               float* dbeta, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_maxpool2_bwd(const float* in, const float* dOut, int C, int D, int H, int W, float* dIn, bfm_stream_t stream);
/* weights of the data-gradient conv: out[ci][co][26-t] = w[co][ci][t], zero rows for Cin <= ci < CinPad */
int bfm_transpose_mirror_weights(const float* w_oidhw, int Cout, int Cin, int CinPad, float* out, bfm_stream_t stream);

/* ---- losses, task-head backward and optimiser step (the rest of one training iteration) -------------------
 * Replaces, for the supervised heads, Trainer/models/criterion.py:111-124,178-186,215-294 + losses.py:10-74 (loss values
 * and, through autograd, their gradients), head.py:52-59 + model.py:207 (1x1x1 heads over F.normalize'd features),
 * torch.optim.AdamW and the clip/unscale reductions of Trainer/engine.py:128-147.
 * raw / dRaw are the head outputs in one of two layouts, told by the strides every loss entry takes: element (column c,
 * voxel v) at raw[c * col_stride + v * voxel_stride] and the same for dRaw.
 *   channels-last [nvox][n_out] (bfm_tail, raw mode):                  col_stride == 1,     voxel_stride == n_out
 *   rows, [n_out] rows of nvox values (bfm_tail_raw_rows; row pitch):  col_stride >= nvox,  voxel_stride == 1
 * Any other pair is BFM_E_ARG.  criterion.py walks one channel of the outputs per loss (outputs[key][:, c], NCDHW in the
 * reference): in rows every access is a contiguous run and the kernels need no LDS staging; the per-voxel expressions are
 * the same code in both layouts (same bits per voxel; the fp64 sums differ by their fold order).  Targets and weights keep
 * the reference's NCDHW layout (one channel = nvox contiguous floats; seg target [ns][nvox]).  Every loss ADDS
 * coef * dL/draw into its columns of dRaw (NULL: value only) and writes the loss value(s) in fp64 (device memory).
 *   l1       mean(|o*m - t*m| * w), l2 flag: mean((o*m - t*m)^2 * w) (bias_field_log_type 'l2'); o clamped to +-clampv first
 *            when clampv > 0 (DistProcessor, no gradient where it clamps); weight w, mask m optional
 *   grad_l1  mean|dx(o) - dx(t)|w + mean|dy ..|w + mean|dz ..|w, forward differences, zero on the last slice
 *   seg      p = softmax(raw[c0:c0+ns]);  loss_out[0] = sum_v CE_v, loss_out[1..ns] = sum_v p t, loss_out[1+ns..] =
 *            sum_v (p+t); gradient of coef_ce * mean_v CE + coef_dice * Dice.  P receives the probabilities in the layout of
 *            raw: [nvox][ns], or [ns] rows of nvox.  Rows: ns <= 64 (BFM_E_SHAPE above). */
size_t bfm_loss_workspace(int ns);
/* n <= 32 l1 / l2 entries of one sample in one pass over raw (host arrays of n columns, l2 flags, clamps, coefficients and
 * device pointers; weights / masks arrays or their elements may be NULL); loss_out [n] (device, fp64 means) */
size_t bfm_loss_l1_multi_workspace(void);
int bfm_loss_l1_multi(const float* raw, int64_t col_stride, int64_t voxel_stride, int n_out, int64_t nvox, int n,
                      const int32_t* cols, const int32_t* l2, const float* clampv, const float* coef,
                      const float* const* targets, const float* const* weights, const float* const* masks, float* dRaw,
                      double* loss_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* every gradient-L1 entry of a sample in one launch: entry k is grad_l1 of column cols[k] against targets[k] [D][H][W] with
 * the optional voxel weight weights[k] (the weight of the voxel a difference is anchored at) and coefficient coef[k];
 * loss_out[k] (device, fp64) = the sum of the three means.  The columns of one call are distinct (two entries on one
 * column would race on dRaw: BFM_E_ARG).  n <= 32; workspace: bfm_loss_l1_multi_workspace(). */
int bfm_loss_grad_l1_multi(const float* raw, int64_t col_stride, int64_t voxel_stride, int n_out, int n, const int32_t* cols,
                           const float* coef, const float* const* targets, const float* const* weights, int D, int H, int W,
                           float* dRaw, double* loss_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_loss_seg(const float* raw, int64_t col_stride, int64_t voxel_stride, int n_out, int c0, int ns, const float* target,
                 const float* wce, const float* wdice, int64_t nvox, float coef_ce, float coef_dice, float* P, float* dRaw,
                 double* loss_out /*[1+2ns]*/, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* Trainer/models/criterion.py:193-212 loss_pathol_ce / loss_pathol_dice on p = sigmoid(raw) (PatholProcessor,
 * Trainer/models/joiner.py:79-87), the one-channel pathology head: ce = mean_v(-log(max(p, 1e-5)) t), dice = 1 - 2 sum(p t) /
 * max(sum(p + t), 1e-5).  The head output of voxel v is raw[col_offset + v * voxel_stride] (channels-last: column, n_out;
 * rows: column * row_stride, 1); dRaw (same addressing, may be NULL) += coef_ce d ce + coef_dice d dice; loss_ce / loss_dice
 * (device fp64; either may be NULL: that loss and its gradient are left out).  Fixed-order fp64 reductions. */
size_t bfm_loss_pathol_workspace(void);
int bfm_loss_pathol(const float* raw, int64_t col_offset, int64_t voxel_stride, const float* target, int64_t nvox,
                    float coef_ce, float coef_dice, float* dRaw, double* loss_ce, double* loss_dice, void* workspace,
                    size_t workspace_bytes, bfm_stream_t stream);
/* Regularisers of the registration head (Trainer/models/losses.py:72-130 SmoothnessLoss('l2') / HessianLoss('l2'), as
 * Trainer/models/criterion.py:187-191 applies them to the raw outputs['registration']).  Field u of nch channels over
 * D x H x W; element (c, v) at raw[col_offset + c * chan_stride + v * voxel_stride] (channels-last: column, 1, n_out; rows:
 * column * row_stride, row_stride, 1).  D_a = forward difference along x (W), y (H) or z (D), zero on the axis' last index.
 *   smooth:  loss_out[0] = mean_{c,v} sum_a (D_a u)^2;  dRaw += coef * (2 / N) sum_a D_a^T D_a u  (N = nch D H W)
 *   hessian: loss_out[0] = SUM_{c,v} det(H)^2, H_ab = D_a D_b u, det as losses.py:136;
 *            dRaw += coef * sum_ab (D_a D_b)^T [2 det ddet/dH_ab]
 * dRaw (same addressing) may be NULL: the value only.  Fixed-order fp64 reductions, no atomics (the same bits on every run).
 * workspace >= bfm_loss_reg_workspace(nch, D, H, W), 8-byte aligned. */
size_t bfm_loss_reg_workspace(int nch, int D, int H, int W);
int bfm_loss_reg_smooth(const float* raw, int64_t col_offset, int64_t chan_stride, int64_t voxel_stride, int nch, int D, int H,
                        int W, float coef, float* dRaw, double* loss_out, void* workspace, size_t workspace_bytes,
                        bfm_stream_t stream);
int bfm_loss_reg_hessian(const float* raw, int64_t col_offset, int64_t chan_stride, int64_t voxel_stride, int nch, int D, int H,
                         int W, float coef, float* dRaw, double* loss_out, void* workspace, size_t workspace_bytes,
                         bfm_stream_t stream);
/* Trainer/models/criterion.py:96-109 loss_feat_contrastive on the feature maps Trainer/models/joiner.py:136-147
 * ContrastiveProcessor leaves (the head-less pre-training mode, Trainer/models/__init__.py:57,169-178): featP / featQ are
 * the RAW last decoder outputs of samples 0 and 1, channels-last [nvox][C] fp32, 2 <= C <= 64; p, q = F.normalize(., dim=1)
 * applied n_norm times (0, 1 or 2: the backbone's unit_feat plus the processor give 2) with eps (1e-12).  Per voxel, with
 * S = sum_j p_j:  num = sum_c exp(p_c q_c / alpha),  den = sum_i [exp(p_i^2 / beta) + exp((p_i S - p_i^2) / gamma)],
 * loss_out[0] (device fp64) = mean_v log(den) - log(num).  Each voxel's largest exponent is subtracted before
 * exponentiating, so the result stays finite where the reference's fp32 overflows and equals it where it does not.
 * dP / dQ [nvox][C] (both or neither; written, not added) = coef * d loss / d featP, d featQ, through the n_norm
 * normalisations; a row whose norm is <= eps is treated as bfm_normalize_bwd treats it: its gradient is the incoming one
 * divided by eps (torch's autograd gives the same 1 / eps there).  coef = loss scale * weight; the loss value does not depend
 * on it.  p_out / q_out [nvox][C] (either may be NULL) receive p and q.  C == 64 with 16-byte aligned maps takes the wide
 * path (8 lanes per voxel, 16-byte accesses); other widths run one wave per voxel.  Fixed-order fp64 reduction, no atomics
 * (the same bits on every run).  workspace >= bfm_loss_contrastive_workspace(), 8-byte aligned. */
size_t bfm_loss_contrastive_workspace(void);
int bfm_loss_contrastive(const float* featP, const float* featQ, int C, int64_t nvox, int n_norm, float eps, float alpha,
                         float beta, float gamma, float coef, float* dP, float* dQ, float* p_out, float* q_out,
                         double* loss_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* dW [n_out][C], db [n_out], dFn [nvox][C] from dRaw [nvox][n_out] and the normalised features Fn [nvox][C] */
size_t bfm_head_bwd_workspace(int n_out, int C, int64_t nvox);
int bfm_head_bwd(const float* dRaw, const float* Fn, const float* head_w, int n_out, int C, int64_t nvox, float* dW,
                 float* db, float* dFn, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* ---- the head outputs as [n_out] ROWS of nvox values (row pitch row_stride >= nvox) instead of channels-last
 * [nvox][n_out]: bfm_tail_raw_rows is TaskHead.forward alone (head.py:52-59) writing that layout, the loss entries above
 * read it by their strides, and bfm_head_bwd_rows (C == 64 and n_out <= 96) is bfm_head_bwd on dRaw in rows. */
int bfm_tail_raw_rows(const float* feat, int64_t nvox, const bfm_tail_desc_t* desc, float* feat_norm, float* raw_rows,
                      int64_t row_stride, bfm_stream_t stream);
int bfm_head_bwd_rows(const float* dRaw_rows, int64_t row_stride, const float* Fn, const float* head_w, int n_out, int C,
                      int64_t nvox, float* dW, float* db, float* dFn, void* workspace, size_t workspace_bytes,
                      bfm_stream_t stream);
/* The heads' backward on a frozen backbone (train.TrainStep(trainable="head")): dW [n_out][C] = dRaw^T . Fn and db [n_out] =
 * the column sums of dRaw, both written; no head weights are read, no dRaw . W product is formed and no [nvox][C] tensor is
 * stored.  Widths as bfm_head_bwd / bfm_head_bwd_rows: the rows form takes C == 64 and n_out <= 96 (BFM_E_SHAPE otherwise;
 * row_stride < nvox: BFM_E_ARG), the channels-last form every C and n_out >= 1.  Exact-fp32 products (fp32-input matrix
 * core), the sum over nvox in a fixed order in two stages through the workspace, no atomics: the same bits on every run, and
 * the same bits from both layouts at C == 64, n_out <= 96.  The bits are not those of bfm_head_bwd's dW. */
size_t bfm_head_wgrad_workspace(int n_out, int C, int64_t nvox);
int bfm_head_wgrad(const float* dRaw, const float* Fn, int n_out, int C, int64_t nvox, float* dW, float* db, void* workspace,
                   size_t workspace_bytes, bfm_stream_t stream);
int bfm_head_wgrad_rows(const float* dRaw_rows, int64_t row_stride, const float* Fn, int n_out, int C, int64_t nvox, float* dW,
                        float* db, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
int bfm_normalize_bwd(const float* feat, const float* dFn, int C, int64_t nvox, float eps, float* dfeat,
                      bfm_stream_t stream);
/* out[0] = sum g^2 (fp64); nonfinite[0] |= 1 when g holds inf/nan (GradScaler.unscale_ / clip_grad_norm_) */
int bfm_grad_sumsq(const float* g, int64_t n, double* out, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                   bfm_stream_t stream);

/* ---- the optimisers of build_optimizer (Trainer/models/__init__.py:360-372; optim.hip) ----------------------------------
 * AdamW, Adam, SGD and LARS over ALL parameters in one launch each, and the clip norms that precede them.  One descriptor per
 * parameter tensor (device memory, 64 bytes): a block owns one chunk (chunk_elems elements, a multiple of 4) of one tensor,
 * chunk_tensor[c] = tensor of chunk c (device), first_chunk = index of the tensor's first chunk.  s0 = exp_avg (Adam, AdamW) |
 * momentum_buffer (SGD) | mu (LARS); s1 = exp_avg_sq (Adam, AdamW; not read by the others, may be NULL).  g is multiplied by
 * grad_scale first (unscale * clip).  bias1 = 1 - beta1^t, bias2_sqrt = sqrt(1 - beta2^t) of the tensor's own step count t
 * (torch's optimisers keep one per parameter; Adam and AdamW alone).  q and wd are LARS' per-tensor trust ratio and weight
 * decay (1 and 0 for a parameter the reference sees as 1-D, utils/misc.py:1299-1310; LARS alone).  16-byte accesses where
 * p, g, s0 (and s1) are all 16-byte aligned and the chunk's length is a multiple of 4, element by element otherwise.  No float
 * atomics: the same bits on every run. */
typedef struct bfm_optim_tensor {
    float* p; const float* g; float* s0; float* s1;
    int64_t n;
    float grad_scale, bias1, bias2_sqrt;
    int32_t first_chunk;
    float q, wd;
} bfm_optim_tensor_t;
/* utils/misc.py:1329-1338 clip_gradients' per-parameter norms: sums_out[t] = sum of squares of tensors[t].g (fp64, fixed
 * order); nonfinite[0] |= 1 when some g holds inf / nan.  Reads g, n and first_chunk alone.  workspace >= nchunks * 8 bytes. */
int bfm_grad_sumsq_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                         int64_t chunk_elems, double* sums_out, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                         bfm_stream_t stream);
/* torch.optim.AdamW of Trainer/models/__init__.py:362-366 (amsgrad off, maximize off; decoupled decay):
 * g = grad_scale g;  p *= 1 - lr wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g g;  p -= (lr / bias1) m / (sqrt(v) / bias2_sqrt
 * + eps), with 1 - beta formed in fp32. */
int bfm_adamw_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                         int64_t chunk_elems, float lr, float beta1, float beta2, float eps, float weight_decay,
                         bfm_stream_t stream);
/* The same step t (1-based) on one flat parameter, bias1 and bias2_sqrt formed here (powf, sqrtf) */
int bfm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, float grad_scale, bfm_stream_t stream);
/* torch.optim.Adam(params_groups) of Trainer/models/__init__.py:361-362 (amsgrad off, maximize off; coupled decay):
 * g = grad_scale g + wd p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g g;  p -= (lr / bias1) m / (sqrt(v) / bias2_sqrt + eps).
 * The betas are doubles so that 1 - beta is rounded to fp32 once, as torch forms it. */
int bfm_adam_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                        int64_t chunk_elems, float lr, double beta1, double beta2, float eps, float weight_decay,
                        bfm_stream_t stream);
/* torch.optim.SGD(params_groups, lr=0, momentum=0.9) of Trainer/models/__init__.py:365-366 (dampening 0, nesterov off):
 * g = grad_scale g + wd p;  buf = momentum buf + g;  p -= lr buf.  A zero buffer gives torch's first step. */
int bfm_sgd_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                       int64_t chunk_elems, float lr, float momentum, float weight_decay, bfm_stream_t stream);
/* What utils.LARS.step (utils/misc.py:1291-1317, Trainer/models/__init__.py:367-368) and clip_gradients (:1329-1338) need of
 * every tensor, from ONE read of p and g: sums_out[3 t + {0, 1, 2}] = sum g^2, sum p^2, sum p g (fp64, fixed order);
 * nonfinite[0] |= 1 when some g holds inf / nan.  workspace >= nchunks * 24 bytes, 8-byte aligned. */
int bfm_lars_sums_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                        int64_t chunk_elems, double* sums_out, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                        bfm_stream_t stream);
/* utils/misc.py:1296-1317 with the norms already taken (q = eta |p| / |dp| or 1, formed by the caller from the sums above):
 * dp = grad_scale g (+ wd p when wd != 0);  dp *= q;  mu = momentum mu + dp;  p -= lr mu */
int bfm_lars_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                        int64_t chunk_elems, float lr, float momentum, bfm_stream_t stream);

/* ------------------------------------------------------------------- pooled scalar (brain-age) head
 * TaskHead's head for out_channels['age'] = -1 (Trainer/models/head.py:39-48 building, :61-66 forward):
 * MaxPool3d(4,4) -> ConvBlock(C_feat->16) -> MaxPool3d(4,4) -> ConvBlock(16->4) -> torch.flatten(x, 1) (NCDHW order)
 * -> final_linear1_age (N->160) + ReLU -> final_linear2_age (160->10) + ReLU -> final_linear3_age (10->1), with
 * ConvBlock = Conv3d(k=3, s=1, p=1, bias) + LeakyReLU(0.2) (head.py:152-167).  Weights in torch's layouts (Conv3d
 * (Cout,Cin,3,3,3), Linear (out,in)); activations channels-last; fp32, no atomics, fixed-order sums (same bits on every
 * run).  The forward is 6 launches, the backward (loss included) 8. */
typedef struct bfm_age_params {
    const float *c1w, *c1b;   /* pool_layers.1.main.{weight,bias}: (16, C_feat, 3,3,3), (16) */
    const float *c2w, *c2b;   /* pool_layers.3.main.{weight,bias}: (4, 16, 3,3,3), (4) */
    const float *l1w, *l1b;   /* final_linear1_age: (160, N), (160) */
    const float *l2w, *l2b;   /* final_linear2_age: (10, 160), (10) */
    const float *l3w, *l3b;   /* final_linear3_age: (1, 10), (1) */
} bfm_age_params_t;
typedef struct bfm_age_grads {
    float *c1w, *c1b, *c2w, *c2b, *l1w, *l1b, *l2w, *l2b, *l3w, *l3b;   /* same shapes as bfm_age_params_t */
} bfm_age_grads_t;
/* nn.MaxPool3d(4, 4) (head.py:40,42; floor mode, no padding) of in (D,H,W,C) -> out (D/4,H/4,W/4,C) plus arg (same shape,
 * bytes): dz*16 + dy*4 + dx of the window's maximum, scanned z, y, x; first maximum on ties, NaN sticky as in nn.MaxPool3d. */
int bfm_maxpool4(const float* in, int C, int D, int H, int W, float* out, uint8_t* arg, bfm_stream_t stream);
/* Its backward (autograd of max_pool3d): g (D/4,H/4,W/4,C) at each window's arg.  accumulate = 0: dst (D,H,W,C) is written
 * whole (0 off the argmax); accumulate = 1: dst[argmax] += g only (one target per window and channel: no atomics). */
int bfm_maxpool4_bwd(const float* g, const uint8_t* arg, int C, int D, int H, int W, float* dst, int accumulate,
                     bfm_stream_t stream);
/* ConvBlock forward (head.py:161-167): y (D,H,W,Cout) = LeakyReLU_0.2(conv3x3x3(x, w, zero padding) + b); Cout % 4 == 0. */
int bfm_age_conv_fwd(const float* x, int Cin, int D, int H, int W, const float* w, const float* b, int Cout, float* y,
                     bfm_stream_t stream);
/* ConvBlock backward: dy = d/dy (after the activation; y = the forward's output, or y = NULL when dy is already the gradient
 * before it) -> dx (D,H,W,Cin) (NULL: not formed), dw (Cout,Cin,3,3,3), db (Cout), all written.  Two launches; the weight
 * gradient is summed per 256 voxels into the workspace and the partials added in order. */
size_t bfm_age_conv_bwd_workspace(int Cin, int D, int H, int W, int Cout);
int bfm_age_conv_bwd(const float* x, int Cin, int D, int H, int W, const float* w, int Cout, const float* y, const float* dy,
                     float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* torch.flatten(x, 1) of the (nv, 4) channels-last conv output (flat index c*nv + voxel) -> the three Linear layers
 * (head.py:64-66): h1 (160), h2 (10) after their ReLU, out[0] = the raw age (before AgeProcessor).  n_flat == 4 * nv, the
 * reference's 4 * s0 // 16 * s1 // 16 * s2 // 16 for a matching size; BFM_E_SHAPE otherwise. */
int bfm_age_mlp_fwd(const float* y2, int nv, const bfm_age_params_t* prm, int n_flat, float* h1, float* h2, float* out,
                    bfm_stream_t stream);
/* Backward of the three Linear layers.  dp_in (device, 1 float) = d/d(raw age); or dp_in = NULL: loss_age of
 * Trainer/criterion.py (| abs(p) - age |, evaluated in float64 -> loss[0] unless NULL) and d/dp = coef * sign(|p| - age) *
 * sign(p) (coef = weight / all_samples * loss scale; 0 at p == 0 or |p| == age, as torch's abs backward).  Writes every
 * final_linear gradient of grd and dy2 (nv, 4) = d/d(conv output).  workspace >= bfm_age_mlp_bwd_workspace(). */
size_t bfm_age_mlp_bwd_workspace(void);
int bfm_age_mlp_bwd(const float* y2, int nv, const bfm_age_params_t* prm, int n_flat, const float* h1, const float* h2,
                    const float* p, const float* dp_in, double age, float coef, double* loss, const bfm_age_grads_t* grd,
                    float* dy2, void* workspace, size_t workspace_bytes, bfm_stream_t stream);

/* ---- hidden task-head layers (task_f_maps longer than one; head_layers.hip) -------------------------------------------
 * Trainer/models/head.py:27-31,52-55,152-167: ConvBlock = Conv3d(f[i], f[i+1], 3, padding 1, bias) + LeakyReLU(0.2), no
 * GroupNorm, between the (normalised, unet3d/model.py:207-208) last feature map and the 1x1x1 heads.  The convolution runs
 * on the existing kernels with the identity affine (scale 1, shift 0, one bound = max |x|) and slope 1; these add the rest.
 * bfm_head_bias_lrelu: y[v][c] = lrelu(y[v][c] + bias[c], slope) in place over (nvox, C) channels-last, C % 4 == 0.
 * mask_image (or NULL; nvox floats): voxels where it is zero are left untouched (a masked convolution leaves boxes of them
 * unwritten).  bound_out (or NULL; device float, zeroed here) = max |y| over the voxels written: the next layer's bound. */
int bfm_head_bias_lrelu(float* y, const float* bias, int C, int64_t nvox, float slope, const float* mask_image,
                        float* bound_out, bfm_stream_t stream);
/* Its backward (autograd over head.py:165-166): dP = dY * (Y > 0 ? 1 : slope), absmax_out (or NULL; zeroed here) = max |dP|,
 * dbias[c] = sum_v dP[v][c] through fp64 partials of fixed voxel ranges folded in ascending order (no atomics: the same bits
 * on every run).  dP may not alias dY.  dW then comes from bfm_conv3x3x3_wgrad_ex and dX from the data-gradient convolution,
 * both with the identity affine.  workspace >= bfm_head_bias_lrelu_bwd_workspace(C, nvox), 8-byte aligned. */
size_t bfm_head_bias_lrelu_bwd_workspace(int C, int64_t nvox);
int bfm_head_bias_lrelu_bwd(const float* dY, const float* Y, int C, int64_t nvox, float slope, float* dP, float* dbias,
                            float* absmax_out, void* workspace, size_t workspace_bytes, bfm_stream_t stream);

/* ---- the evaluator (Trainer/models/evaluator.py; eval_metrics.hip) ----------------------------------------------------
 * Volumes are contiguous fp32 (or int32 labels), planes = B * C.  Every workspace and every fp64 / int64 output is 8-byte
 * aligned device memory.  Sums are fp64 block partials folded in a fixed order (no float atomics: the same bits on every
 * run); nothing is written when a call is rejected.
 *
 * get_l1 / get_psnr / get_normalized_l2 (evaluator.py:100-119) and the min / max of get_ssim / get_ms_ssim (:125-126,
 * :134-135) from one read of o (output) and t (target): stats[0..9] = sum|o-t|, sum(o-t)^2, sum(o t), sum(o^2), sum(t^2),
 * min o, max o, min t, max t, count(t != 0); differences and products are formed in fp64.  Min and max propagate NaN as
 * torch's do.  The scores are host arithmetic on these numbers. */
size_t bfm_eval_pair_stats_workspace(void);
int bfm_eval_pair_stats(const float* o, const float* t, int64_t n, double* stats /*[10]*/, void* workspace,
                        size_t workspace_bytes, bfm_stream_t stream);
/* get_l1(nonzero_only=True), evaluator.py:106-108: the reference sums over dim 0, the batch, so the result is a volume:
 * out[i] = sum_b |t[b][i] - o[b][i]| [t[b][i] != 0] / sum_b [t[b][i] != 0] in fp32 (NaN where no sample's target is
 * non-zero); n = elements per sample. */
int bfm_eval_l1_nonzero(const float* o, const float* t, int B, int64_t n, float* out, bfm_stream_t stream);
/* get_dice on probability maps, evaluator.py:96-97: out[p] = {sum(o t), sum(o + t)} over plane p's n_per voxels. */
size_t bfm_eval_channel_sums_workspace(int planes, int64_t n_per);
int bfm_eval_channel_sums(const float* o, const float* t, int planes, int64_t n_per, double* out /*[planes][2]*/,
                          void* workspace, size_t workspace_bytes, bfm_stream_t stream);
/* get_onehot + get_dice on two label maps (evaluator.py:30-40,96-97,170-172) without the one-hot: with c = lut[label],
 * counts[l] = |{P: c == l}|, counts[n_labels + l] = |{T: c == l}|, counts[2 n_labels + l] = |{both}|, and
 * counts[3 n_labels] = how many labels of P and T lie outside [0, nlut) (the reference's LUT indexing raises IndexError
 * there; a lut entry outside [0, n_labels) counts the same way) -- such voxels enter no class.  counts is zeroed by the call.
 * Integer LDS histograms and integer global adds: exact in any order.  n_labels <= 256, n <= 2^40 (BFM_E_SHAPE). */
int bfm_eval_label_counts(const int32_t* P, const int32_t* T, int64_t n, const int32_t* lut, int nlut, int n_labels,
                          int64_t* counts /*[3 n_labels + 1]*/, bfm_stream_t stream);
/* pytorch_msssim 1.0's _ssim on (planes, D, H, W) volumes (get_ssim / get_ms_ssim, evaluator.py:121-141; data range 1,
 * K = (0.01, 0.03)): the 11-tap window win_host (host, fp32, sums to 1) filters X, Y, XX, YY, XY "valid" along every axis
 * of length >= 11 (a shorter axis is left unfiltered at full length), then
 *   cs = (2 s12 + C2) / (s1 + s2 + C2),  ssim = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1) * cs,
 * out[p] = {mean ssim, mean cs} of plane p (fp64 sums of the fp32 maps).  The filtered moments never leave the CU.
 * norm_dev (or NULL) = {min X, max X, min Y, max Y} on the device: each value is read as (x - min) / (max - min), fp32, a
 * true division -- a constant volume gives NaN, as the reference does.  H * W < 2^31, planes <= 65535 (BFM_E_SHAPE). */
size_t bfm_eval_ssim3d_workspace(int planes, int D, int H, int W);
int bfm_eval_ssim3d(const float* X, const float* Y, int planes, int D, int H, int W, const float* win_host /*[11]*/,
                    const double* norm_dev /*[4] or NULL*/, double* out /*[planes][2]*/, void* workspace,
                    size_t workspace_bytes, bfm_stream_t stream);
/* The pooling between the scales of pytorch_msssim's ms_ssim: F.avg_pool3d(kernel 2, padding n % 2 per axis), padded
 * zeros counted in the divisor, of X and Y in one launch: outputs (planes, (D+1)/2, (H+1)/2, (W+1)/2).  norm_dev as above
 * (scale 0 reads the raw volumes). */
int bfm_eval_avgpool2_pair(const float* X, const float* Y, int planes, int D, int H, int W,
                           const double* norm_dev /*[4] or NULL*/, float* Xo, float* Yo, bfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BRAINFM_HIP_H */
