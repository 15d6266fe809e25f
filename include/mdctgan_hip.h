/* libmdctgan_hip.so -- C ABI of the MI355X (gfx950) mdctGAN hot path.
 *
 * The reference (neoncloud/mdctGAN) is pure Python/PyTorch and has no FFI layer of its own: the
 * seam is the module API of models/mdct.py, models/pix2pixHD_model.py and models/networks.py.
 * Each entry point below replaces the chain of ATen ops one of those methods dispatches; the
 * reference site it replaces is cited on every declaration (paths relative to the reference
 * repository).  The Python package mdctgan_amd binds these with ctypes and re-exposes the reference's own
 * class / function names (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless it says "host"; no torch types anywhere;
 *   - activations are float32 NHWC ([B, H, W, C], C fastest); spectrograms [B, F, 256] are the
 *     C == 1 case of both NHWC and the reference's NCHW;
 *   - convolution weights are float32 "OHWI": [Cout, KH, KW, Cin] for nn.Conv2d and
 *     [Cin_T, KH, KW, Cout_T] for nn.ConvTranspose2d.  A reference-shaped state_dict tensor
 *     ([Cout, Cin, KH, KW] / [Cin_T, Cout_T, KH, KW]) is the SAME memory viewed through
 *     .permute(0, 3, 1, 2), so checkpoints load unchanged;
 *   - `stream` is a hipStream_t (0 = the null stream); all work is enqueued asynchronously;
 *   - return value: 0 on success, a positive hipError_t, or MG_ERR_* (negative) for a rejected
 *     argument.  Nothing is ever computed on the host.
 */
#ifndef MDCTGAN_HIP_H
#define MDCTGAN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_ERR_ARG (-1)
#define MG_ERR_UNSUPPORTED (-2)

/* codec selector: raw MDCT coefficients, arcsinh + range-norm, range-norm only (--raw_mdct) */
#define MG_CODEC_RAW 0
#define MG_CODEC_ARCSINH 1
#define MG_CODEC_RANGE 2

/* activation selector for fused epilogues */
#define MG_ACT_NONE 0
#define MG_ACT_RELU 1
#define MG_ACT_LRELU02 2
#define MG_ACT_TANH 3

/* 3 since mg_mdct4_forward / mg_imdct4_forward take the factored DCT-IV image (dct4_image) in the middle of their argument lists: a
   caller built against an older header must see a different number here before it passes `codec` where a pointer is expected.
   4 (round 6): mg_grad_seg / mg_scaler_check_segs / mg_adam_step_segs / mg_conv_wgrad_h16 added; mg_conv_wgrad_chk's found_inf
   test uses float16's overflow criterion (|v| >= 65520), as the --fp16 optimiser passes do. */
int mg_abi_version(void);
/* sizeof(mg_conv_geom) as the library was built (13 ints = 52 bytes): a binding checks its own struct against it */
int mg_conv_geom_size(void);

/* ------------------------------------------------------------------------------------------
 * K1  MDCT4.forward (models/mdct.py:392-425) fused with Audio2MDCT.normalize
 *     (models/pix2pixHD_model.py:83-125) and the 2-channel input build (:400-402).
 *
 *   audio [B, T] -> spec [B, F, n_fft/2], F = mg_mdct4_num_frames(T, n_fft); n_fft == 512 (hop 256).
 *   codec RAW: spec = X.  ARCSINH: L = asinh(gain*X)/ln10.  RANGE: L = X.  Then
 *   spec = (L - min)/(max - min)*(nr1 - nr0) + nr0, with (min, max) = (src_min, src_max)
 *   (--abs_norm) or, when per_sample != 0, the per-clip min/max of L (written to min_out/max_out [B]).
 *   in2 (nullable): NHWC pair [B, F, 256, 2] = (spec, 2*|spec| + nr0) -- the generator input.
 *   frames_out (nullable): windowed frames [B, F, n_fft] (return_frames=True).
 *   stats (nullable): double[2] = sum(L), sum(L^2) over the batch (for the returned mean / std).
 *   scratch_u32: >= 2*B uint32, required when per_sample != 0.
 *   window [n_fft] and dct4 [n_fft/2][n_fft/2] = cos(pi/M (n+1/2)(k+1/2)) are device tables.
 *   dct4_image (nullable): mg_dct4_image_floats(n_fft) floats that mg_dct4_image(dct4, dct4_image, stream) fills once per
 *   table -- the operand images the table-stationary kernels keep in registers (csrc/mdct_bs.h: the float32 register image;
 *   csrc/mdct_b3.h: three bf16 piece images, the float32 value being their exact sum).  NULL selects the kernels that read
 *   the plain table only (a caller written against the round-1 ABI passes its m*m table and NULL).  16-byte aligned.
 *   spec may be NULL when in2 is given and the table-stationary kernels apply (dct4_image present, T % 4 == 0, 16-byte aligned
 *   pointers, no per_sample, no frames_out; MG_ERR_ARG otherwise): the spectrogram is then channel 0 of the pair only
 *   (393 216 B per clip moved instead of 526 848).
 */
long long mg_dct4_image_floats(int n_fft);
int mg_dct4_image(const float* dct4, float* dct4_image, void* stream);
int mg_mdct4_forward(const float* audio, int B, int T, int n_fft, const float* window, const float* dct4,
                     const float* dct4_image, int codec, float gain, float nr0, float nr1, float src_min, float src_max,
                     int per_sample, float* spec, float* in2, float* frames_out, float* min_out, float* max_out,
                     double* stats, unsigned* scratch_u32, void* stream);
int mg_mdct4_num_frames(int T, int n_fft);

/* K2  Audio2MDCT.denormalize (models/pix2pixHD_model.py:127-137) fused with IMDCT4.forward
 *     (models/mdct.py:457-489: inverse DCT, window, fold() overlap-add, 4/N scale, centre crop).
 *   spec [B, F, 256] -> audio [B, out_len], out_len <= (F-1)*256; float32, or float64 when out_f64.
 *   min_b / max_b (nullable, [B]): per-clip range; otherwise (src_min, src_max).
 *   frames_out (nullable): windowed synthesis frames [B, F, n_fft].
 */
int mg_imdct4_forward(const float* spec, int B, int F, int n_fft, const float* window, const float* dct4,
                      const float* dct4_image, int codec, float gain, float nr0, float nr1, float src_min, float src_max,
                      const float* min_b, const float* max_b, void* audio, int out_len, int out_f64,
                      float* frames_out, void* stream);

/* K2 + generate_audio.py:40-53 in ONE kernel: IMDCT4.forward whose overlap-add store writes straight into the stitched waveform,
 *     replacing `audio.append(sr_audio)` (generate_audio.py:37), the two `*= 0.5`, F.fold and the final crop (generate_audio.py:
 *     43-50) -- and torch.cat(...).view(1, -1) (generate_audio.py:52) when gen_overlap == 0.
 *   spec [B, F, 256] are segments first_seg .. first_seg + B - 1 of a signal cut into segments of seg_len samples at stride
 *   seg_len - overlap (data/audio_dataset.py:153-167 seg_pad_audio); out is the WHOLE stitched waveform, out_total =
 *   mg_stitch_length(n_seg, seg_len, overlap) samples.  Sample t of segment s lands at s * (seg_len - overlap) - overlap + t
 *   (positions outside [0, out_total) are the reference's crop); the first / last `overlap` samples of every segment are halved
 *   and added to the neighbour's (two-term float sums: order-free, equal to F.fold's bit for bit), the rest is stored.  So with
 *   overlap > 0 the waveform must be zero before the first batch writes: zero_out != 0 makes this call clear it first
 *   (a memset node in front of the kernel: pass it for the batch with first_seg == 0).  Batches may arrive in any order.
 *   float32 output (float64 when out_f64 -- generic kernel); seg_len <= (F-1)*256.  Same codec arguments as mg_imdct4_forward.
 */
int mg_imdct4_stitched(const float* spec, int B, int F, int n_fft, const float* window, const float* dct4,
                       const float* dct4_image, int codec, float gain, float nr0, float nr1, float src_min, float src_max,
                       const float* min_b, const float* max_b, void* out, long long out_total, int seg_len, int overlap,
                       long long first_seg, int zero_out, int out_f64, void* stream);

/* Row tables: batched inference over utterances of different lengths (segments of any number of utterances share a batch).
 *   mg_seg_row (a DEVICE array, one entry per batch row): sample t of row r is index p = pos + t of a packed buffer that holds all
 *   utterances; the sample exists only if lo <= p < hi ([lo, hi) is the row's utterance); lo == hi marks a dead row.  pos may be
 *   negative or anything else: only positions inside the window are touched (a window that sticks out of the buffer is cut to it).
 *   mg_segments_gather       data/audio_dataset.py:153-167 (seg_pad_audio: pad + unfold) from the packed waveform `wave`
 *                            [wave_total]: out[r][t] = (lo <= pos + t < hi) ? wave[pos + t] : 0 for out [n_rows, seg_len]; dead rows
 *                            come out as zeros.  16-byte loads where pos and the pointers allow, scalar loads otherwise.  No atomics.
 *   mg_imdct4_stitched_rows  mg_imdct4_stitched with `rows` [B] in place of first_seg; out / out_total are the whole packed buffer.
 *                            Per row the semantics of mg_imdct4_stitched with the row's window in place of [0, out_total): sample t
 *                            lands at pos + t and is dropped outside [lo, hi) (the reference's final crop), the first / last
 *                            `overlap` samples of every segment are halved and added (so the windows must be zero beforehand when
 *                            overlap > 0), the rest is stored; a dead row writes nothing; nothing outside the windows is written.
 *                            zero_out != 0 clears the whole packed buffer first (a memset node).  The same kernels as
 *                            mg_imdct4_stitched by the same guards (overlap % 4 == 0 for the factored one), so a row table that
 *                            describes one utterance gives that call's bits; 16-byte stores where pos % 4 == 0.
 *   mg_imdct4_pow2_stitched_rows  the same for mg_imdct4_pow2_stitched (n_fft 256 / 1024 / 2048, float32).
 *   mg_mdct_last_kernel(1) names the variants "...<stitched rows> ...". */
typedef struct { long long pos, lo, hi; } mg_seg_row;
int mg_segments_gather(const float* wave, long long wave_total, const mg_seg_row* rows, int n_rows, int seg_len, float* out,
                       void* stream);
int mg_imdct4_stitched_rows(const float* spec, int B, int F, int n_fft, const float* window, const float* dct4,
                            const float* dct4_image, int codec, float gain, float nr0, float nr1, float src_min, float src_max,
                            const float* min_b, const float* max_b, void* out, long long out_total, int seg_len, int overlap,
                            const mg_seg_row* rows, int zero_out, int out_f64, void* stream);
int mg_imdct4_pow2_stitched_rows(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                                 float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b,
                                 const float* max_b, void* out, long long out_total, int seg_len, int overlap,
                                 const mg_seg_row* rows, int zero_out, int out_f64, void* stream);

/* Which kernel the last mg_mdct4_forward (which == 0) / mg_imdct4_forward / mg_imdct4_stitched (which == 1) call of this process
 * launched -- a static string ("mdct4_ct_kernel (csrc/mdct_ct.h)", ...).  Diagnostic: bench.py names the measured kernel with it. */
const char* mg_mdct_last_kernel(int which);

/* Backward passes of K2 / K1 (gradients through Audio2MDCT.to_audio / to_spectro and the raw IMDCT4 / MDCT4), n_fft = 512.
 *   mg_imdct4_backward  grad_audio [B, out_len] (the gradient of K2's output) -> grad_spec [B, F, 256]
 *                       = dX/ds(spec) * 4/N * MDCT(grad_audio), frames taken as K1 takes them with F frames, grad_audio zero past
 *                       out_len (out_len <= (F-1)*256).  Same codec arguments as mg_imdct4_forward (RAW: spec may be NULL;
 *                       min_b / max_b [B]: per-clip range, used as constants).
 *   mg_mdct4_backward   grad_spec [B, F, 256] (the gradient of K1's normalised output spec) -> grad_audio [B, T]
 *                       = N/4 * IMDCT(ds/dX(spec) * grad_spec) cropped to T, F = mg_mdct4_num_frames(T, 512); fixed range only.
 *   dX/ds = c1 cosh(c1 s + c0) / gain (arcsinh), c1 (range), 1 (raw), c1 = ln10^[arcsinh] (max - min) / (nr1 - nr0) and
 *   c0 = ln10^[arcsinh] (min - nr0 (max - min) / (nr1 - nr0)).  Deterministic (no atomics).  MG_ERR_UNSUPPORTED where the
 *   factored kernels' guards fail (no dct4_image, T or out_len % 4, unaligned or > 4 GiB operands, MG_MDCT_CT=0 / MG_MDCT_FT):
 *   the caller then composes mg_frames_window / mg_conv_fwd / mg_codec_backward / mg_overlap_add.  mg_mdct_last_kernel is not
 *   touched. */
int mg_imdct4_backward(const float* grad_audio, int B, int out_len, int F, int n_fft, const float* window, const float* dct4_image,
                       int codec, float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b,
                       const float* max_b, const float* spec, float* grad_spec, void* stream);
int mg_mdct4_backward(const float* grad_spec, const float* spec, int B, int T, int n_fft, const float* window, const float* dct4_image,
                      int codec, float gain, float nr0, float nr1, float src_min, float src_max, float* grad_audio, void* stream);

/* K1' / K2' (csrc/mdct_pow2.hip): the fused transform + codec kernels of the power-of-two geometries other than 512:
 *   win_length == n_fft == 2 * hop_length, centre padding, n_fft in {256, 1024, 2048}.  TDAC fold + DCT-IV as an n_fft/4-point
 *   complex FFT between two twiddles (plain float32, radix-4 Stockham stages in LDS); the frames never travel through HBM.
 *   mg_mdct_pow2_supported   1 when (n_fft, hop_length, win_length, center) is such a geometry, else 0 (n_fft == 512 belongs to
 *                            K1 / K2: 0).  Pure host query.
 *   mg_mdct_pow2_twiddle_floats / mg_mdct_pow2_twiddles   the twiddle buffer the three calls below read: 3 * n_fft/2 floats =
 *                            [pre | post | root], n_fft/4 interleaved complex each: pre[n] = exp(-i pi (4n+1) / (2 n_fft)),
 *                            post[k] = exp(-i pi 4k / (2 n_fft)), root[t] = exp(-i pi 16t / (2 n_fft)).  Filled on the HOST into
 *                            `out` (float32, or float64 when as_f64: the values before their one rounding); the caller copies
 *                            the float32 form to the device once per geometry (not inside a graph capture).  16-byte aligned.
 *   mg_mdct4_pow2_forward    audio [B, T] -> spec [B, F, n_fft/2] with mg_mdct4_forward's codec arguments (RAW / ARCSINH / RANGE
 *                            with the fixed range; stats as there).  F is the caller's: mg_mdct4_num_frames(T, n_fft) for
 *                            MDCT4.forward; frame f covers samples (f-1) hop .. (f+1) hop - 1, zeros outside [0, T).  Any T.
 *                            per_sample != 0, frames_out != NULL, an unaligned spec: MG_ERR_UNSUPPORTED.
 *   mg_imdct4_pow2_forward   spec [B, F, n_fft/2] -> audio [B, out_len] float32, out_len <= (F-1) hop, with mg_imdct4_forward's
 *                            codec arguments; out_scale replaces the transform's 4 / n_fft (the adjoint of K1' is K2' with scale 1).
 *                            No atomics: identical bits run to run.  out_f64 != 0, an unaligned spec: MG_ERR_UNSUPPORTED.
 *   mg_imdct4_pow2_stitched  mg_imdct4_stitched's arguments and semantics on these geometries (float32 only); equal to
 *                            mg_imdct4_pow2_forward followed by mg_stitch_segments bit for bit.
 *   MG_ERR_UNSUPPORTED sends the caller to the composition (mg_frames_window / mg_conv_fwd / mg_codec_* / mg_overlap_add).
 *   mg_mdct_last_kernel(0 | 1) names these kernels after the calls ("mdct4_pow2_kernel ...", "imdct4_pow2_kernel ...",
 *   "imdct4_pow2_kernel<stitched> ..."). */
int mg_mdct_pow2_supported(int n_fft, int hop_length, int win_length, int center);
long long mg_mdct_pow2_twiddle_floats(int n_fft);
int mg_mdct_pow2_twiddles(int n_fft, void* out, int as_f64);
int mg_mdct4_pow2_forward(const float* audio, int B, int T, int F, int n_fft, const float* window, const float* twiddles, int codec,
                          float gain, float nr0, float nr1, float src_min, float src_max, int per_sample, float* spec,
                          float* frames_out, double* stats, void* stream);
int mg_imdct4_pow2_forward(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                           float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b,
                           void* audio, int out_len, int out_f64, float out_scale, void* stream);
int mg_imdct4_pow2_stitched(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                            float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b,
                            void* out, long long out_total, int seg_len, int overlap, long long first_seg, int zero_out,
                            int out_f64, void* stream);

/* F1  torchaudio.functional.resample(waveform, orig_freq, new_freq) with its defaults (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99) as the reference's data path calls it (data/audio_dataset.py:66-71, 171-177):
 * x [B, L] -> out [B, mg_resample_length(L, orig, new)], orig / new the gcd-reduced rates.  kern [new, 2*width + orig]
 * is the polyphase filter bank torchaudio's _get_sinc_resample_kernel builds (the host computes it once per rate pair
 * in float64 and passes it in float32, as torchaudio does). */
long long mg_resample_length(long long L, int orig, int new_);
int mg_resample(const float* x, int B, int L, const float* kern, int orig, int new_, int width, float* out, int out_len,
                void* stream);

/* The same data path for MANY utterances in shared launches (data/audio_dataset.py:66-78 and 141-186, --add_noise included):
 * every utterance sits at its own place of one packed buffer, device row tables (arrays of long long, as mg_seg_row) say where
 * each row reads and writes.  Windows are cut to their buffers inside the kernels (a bad table drops samples, it never touches
 * memory outside them), a row of length 0 is a dead row, there are no atomics and every sum has one fixed order: an utterance has
 * the same bits alone as inside any pack.  No host synchronisation; the launch count does not depend on n_rows.
 *   mg_resample_rows   mg_resample over a packed buffer: row u reads x[in_pos, in_pos + in_len) and writes out[out_pos, out_pos +
 *                      out_len), out_len = mg_resample_length(in_len, orig, new_) (the host builds the table so), one call per
 *                      rate pair.  max_out_len (the longest out_len, known to the host) only sizes the grid.  shift [n_rows] or NULL:
 *                      row u's samples enter as x + shift[u] (a float32 add; the zero padding around the row stays zero) -- the
 *                      `raw += 1e-4 - mean(raw)` of :146.  Per output sample the fmaf chain of mg_resample in ascending tap order:
 *                      bit-identical to mg_resample on the row alone (on x + shift with a shift).  Rows longer than INT_MAX are
 *                      dropped.  Filter banks above 48 KB stay in global memory, as in mg_resample.
 *   mg_rows_moments    out[r] = {sum x, sum x^2} (double) over the window [lo, hi) of rows[r] (pos is not used): chunks of
 *                      MG_MOMENTS_CHUNK samples counted from lo, each summed by one workgroup in a fixed tree, then the chunks in
 *                      ascending order.  max_len: the longest window (sizes the workspace and the grid; longer rows lose their
 *                      tail).  workspace: mg_rows_moments_workspace(n_rows, max_len) bytes.  A dead row gives {0, 0}.
 *   mg_add_noise_rows  :73-78 / :179-184 per row, in place on the packed low-rate buffer: lr = lr + a (noise - m) in float32, with
 *                      m = sum n / N and a = sqrt((sum lr^2 / segment_length) / 10^(snr / 10)) / std(n) computed on the device
 *                      from the two mg_rows_moments results; std is the unbiased one (N - 1), and the divisor of the signal
 *                      power is segment_length, not N, as in the reference.  noise has lr's layout.  Rows of fewer than 2 samples
 *                      are left alone (the caller refuses them). */
#define MG_MOMENTS_CHUNK 4096
typedef struct { long long in_pos, in_len, out_pos, out_len; } mg_resample_row;
int mg_resample_rows(const float* x, long long x_total, const mg_resample_row* rows, int n_rows, long long max_out_len,
                     const float* shift, const float* kern, int orig, int new_, int width, float* out, long long out_total,
                     void* stream);
size_t mg_rows_moments_workspace(int n_rows, long long max_len);
int mg_rows_moments(const float* x, long long total, const mg_seg_row* rows, int n_rows, long long max_len, double* out,
                    void* workspace, size_t workspace_bytes, void* stream);
int mg_add_noise_rows(float* lr, const float* noise, long long total, const mg_seg_row* rows, int n_rows, long long max_len,
                      const double* lr_moments, const double* noise_moments, double snr, long long segment_length, void* stream);

/* The TRAINING side of that data path (data/audio_dataset.py:34-82, AudioDataset.readaudio + __getitem__) for a whole batch in shared
 * launches (csrc/train_rows.hip): the corpus sits packed in one float32 device buffer, a device row table (one mg_train_row per batch
 * row) names the window every row loads, and (LR_audio, HR_audio) come out as two dense [out_rows, seg_len] tensors.
 *   mg_resample_bank    one polyphase filter bank as mg_resample takes it (kern [new_, 2*width + orig], gcd-reduced rates);
 *                       kern == NULL: equal rates, the step is a copy (orig / new_ / width are not read).
 *   mg_train_row        the row loads corpus[in_pos, in_pos + in_len) -- torchaudio.load(frame_offset, num_frames) -- and writes row
 *                       out_row of lr and hr; in_len == 0 marks a dead row, which writes nothing.  full_pos / full_len are read only
 *                       with lr_full.  The window is the WHOLE signal in both legs: taps outside it contribute nothing, whatever
 *                       the corpus holds next to it (another file's samples, or the same file's).
 *   mg_train_pair_rows  hr[out_row][t] = resample(window, to_hr)[t] for t < min(seg_len, ceil(hr L / fs)), zero after;
 *                       lr[out_row][t] = resample(resample(window, to_lr), lr_to_hr)[t] for t < min(seg_len, ceil(hr M / lr)),
 *                       M = ceil(lr L / fs), zero after (seg_pad_audio, :102-110; the two lengths differ in general).  Two launches,
 *                       whatever n_rows is: the hr leg, and the lr leg as ONE kernel -- a workgroup computes the lr-rate samples
 *                       its tile of outputs touches into LDS (each rounded to float32 once, as the tensor between the two
 *                       aF.resample calls; none beyond M) and runs the second chain from there.  Every chain is mg_resample's fmaf
 *                       chain in ascending tap order: a row has the bits of mg_resample (twice) on its window alone, whatever else
 *                       shares the launch.  Banks of more than 2048 floats are read from global memory; LDS is static (32 KB), so
 *                       nothing is configured before a graph capture.  No atomics, no host synchronisation.
 *                       lr_full != NULL (--add_noise, whose power and standard deviation run over the signal BEFORE the crop,
 *                       :72-78): the lr leg writes the whole low-rate signal of row u to lr_full[full_pos, full_pos + full_len)
 *                       (full_len = ceil(hr M / lr), the host builds the table so; max_full_len, the longest, sizes the grid) and
 *                       leaves lr alone (it may be NULL); mg_rows_moments, mg_add_noise_rows and mg_segments_gather finish the batch.
 *                       Windows that stick out of the corpus are cut to it; rows whose out_row or lr_full window lies outside
 *                       their buffers, or longer than 2^30 samples, are dropped.  MG_ERR_ARG: a null pointer, n_rows, seg_len,
 *                       corpus_total or out_rows <= 0, a malformed bank.  MG_ERR_UNSUPPORTED: an lr_to_hr bank whose taps of one
 *                       output sample do not fit the 4096 intermediates a tile holds. */
typedef struct { const float* kern; int orig, new_, width; } mg_resample_bank;
typedef struct { long long in_pos, in_len, out_row, full_pos, full_len; } mg_train_row;
int mg_train_pair_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                       const mg_resample_bank* to_hr, const mg_resample_bank* to_lr, const mg_resample_bank* lr_to_hr, float* lr,
                       float* hr, long long out_rows, float* lr_full, long long lr_full_total, long long max_full_len,
                       void* stream);
/*   mg_train_hr_rows / mg_train_lr_rows   the two legs of mg_train_pair_rows as entry points of their own: the same kernels on the
 *                       same grids, hence the same bits, lr_full included.  For a batch whose low-rate leg reads another buffer
 *                       than its high-rate leg (the low-pass augmentation below filters the windows into a scratch buffer first):
 *                       neither leg is computed twice.  Arguments and refusals as in mg_train_pair_rows. */
int mg_train_hr_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                     const mg_resample_bank* to_hr, float* hr, long long out_rows, void* stream);
int mg_train_lr_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                     const mg_resample_bank* to_lr, const mg_resample_bank* lr_to_hr, float* lr, long long out_rows, float* lr_full,
                     long long lr_full_total, long long max_full_len, void* stream);

/* Low-pass rows (csrc/sos_rows.hip): an IIR filter given as a cascade of second-order sections over the rows of a packed buffer,
 * one pass or forward-backward (zero phase) -- a different anti-aliasing filter per training example before the rate change
 * (lowpass.py designs Butterworth and Chebyshev-I filters; not in the reference).
 *   mg_sos_row    the row reads x[in_pos, in_pos + len) and writes out[out_pos, out_pos + len); len == 0 marks a dead row.
 *   sos           double [n_rows][MG_SOS_MAX_SECTIONS][6] on the device: b0 b1 b2 a0 a1 a2 per section, a0 == 1 (it is not
 *                 read); an unused section is the identity 1 0 0 1 0 0.  The caller checks stability (|a2| < 1, |a1| < 1 + a2).
 *   mg_sos_rows   y = cascade(x) from a zero state in double; zero_phase != 0: then the cascade again, from a zero state, over the
 *                 reversed result, the value in between kept in double -- sosfilt(sos, sosfilt(sos, x)[::-1])[::-1] in float64,
 *                 rounded to float32 once.  The signal is zero outside the row's window (cut to x); every store is guarded.
 *                 Parallel inside a row: chunks of MG_SOS_CHUNK samples, counted from the row's first sample (from its last in the
 *                 reverse pass), each run from a zero state; the true start states are carried along the row in ascending chunk
 *                 order with the chunk transition matrix (taken on the device from zero-input runs); the chunks are run again
 *                 from them.  No atomics, every sum has one fixed order: a row has the same bits alone as inside any pack, in any
 *                 order, run to run.  3 launches (6 with zero_phase) whatever n_rows is; static LDS, no host synchronisation.
 *                 max_len: the longest row (at most 2^30); longer rows are dropped.  workspace: mg_sos_rows_workspace(n_rows,
 *                 max_len) bytes, 8-byte aligned (0: invalid arguments).  MG_ERR_ARG before any launch: a null pointer, n_rows,
 *                 x_total, out_total or max_len <= 0, a short workspace, out overlapping x. */
#define MG_SOS_MAX_SECTIONS 6
#define MG_SOS_CHUNK 256
typedef struct { long long in_pos, len, out_pos; } mg_sos_row;
size_t mg_sos_rows_workspace(int n_rows, long long max_len);
int mg_sos_rows(const float* x, long long x_total, const mg_sos_row* rows, const double* sos, int n_rows, long long max_len,
                int zero_phase, float* out, long long out_total, void* workspace, size_t workspace_bytes, void* stream);

/* WAV payloads (csrc/pcm_rows.hip): torchaudio.load(normalize=True) (data/audio_dataset.py:37-51, :143) and torchaudio.save
 * (generate_audio.py:89-96) for MANY files in shared launches.  The payload bytes of every file sit in one byte buffer (the host
 * stages each at a 16-byte aligned offset), the waveforms in one packed float32 buffer; one mg_pcm_row per channel of a file.
 *   mg_pcm_row          decode: the row reads channel `channel` of `frames` interleaved little-endian frames of `channels` samples
 *                       that start at byte src_pos, and writes float32 samples to out[dst_pos, dst_pos + frames).  encode: src_pos
 *                       is the sample position of this channel's row in x, dst_pos the byte offset of the file's payload.
 *   mg_pcm_decode_rows  U8: (x - 128) / 128.  S16, S24: x / 2^(bits - 1), exact.  S32: float32(x) 2^-31 -- one round to nearest even,
 *                       then an exact scale.  F32: the bits as they are, NaNs included.  F64: one round-to-nearest-even cast.  One
 *                       workgroup per chunk of MG_MOMENTS_CHUNK frames of a row.  moments != NULL: double [n_rows][2] = {sum x,
 *                       sum x^2} of every decoded row from the same pass, bit for bit mg_rows_moments over out[dst_pos, dst_pos +
 *                       frames) with the same max length (one small launch more); workspace: mg_pcm_decode_rows_workspace(n_rows,
 *                       max_frames) bytes, 8-byte aligned, read only with moments.  max_frames: the longest row (sizes the grid and
 *                       the workspace; longer rows lose their tail).
 *   mg_pcm_encode_rows  MG_PCM_F32: a bit copy.  MG_PCM_S16 / MG_PCM_S24: clamp(rint(x 2^(bits - 1)), -2^(bits - 1), 2^(bits - 1) - 1),
 *                       round half to even, the product exact, NaN -> 0.  clipped [n_rows]: per row the samples that were clamped or
 *                       NaN (0 for F32).  The rows of one file write disjoint bytes of the same frames.  One workgroup per row.  A
 *                       row of any other format is a dead row here (the table lives on the device): the binding refuses it with
 *                       MG_ERR_UNSUPPORTED's exception before the launch.  No dither.
 * A row is cut to both of its buffers in whole frames: no load or store touches a byte outside [0, bytes_total) or a sample outside
 * the float buffer.  A row with frames <= 0, a negative or too large position, channels outside [1, 65535], channel outside
 * [0, channels) or an unknown format is dead (decode writes nothing and gives moments {0, 0}; encode gives clipped 0).  No atomics,
 * every sum has one fixed order: a row has the same bits alone as inside any pack.  No host synchronisation; the launch count
 * does not depend on n_rows.  MG_ERR_ARG before any launch: a null pointer, n_rows, a total or max_frames <= 0, a short workspace. */
#define MG_PCM_U8 0
#define MG_PCM_S16 1
#define MG_PCM_S24 2
#define MG_PCM_S32 3
#define MG_PCM_F32 4
#define MG_PCM_F64 5
typedef struct { long long src_pos, frames, channels, channel, format, dst_pos; } mg_pcm_row;
size_t mg_pcm_decode_rows_workspace(int n_rows, long long max_frames);
int mg_pcm_decode_rows(const void* bytes, long long bytes_total, const mg_pcm_row* rows, int n_rows, long long max_frames,
                       float* out, long long out_total, double* moments, void* workspace, size_t workspace_bytes, void* stream);
int mg_pcm_encode_rows(const float* x, long long x_total, const mg_pcm_row* rows, int n_rows, long long max_frames, void* bytes,
                       long long bytes_total, long long* clipped, void* stream);

/* F2  util/util.py:132-177 compute_matrics on the device (train.py:104-134 eval_model, generate_audio.py:60).
 *   mg_metrics_rows   out[b] = {sum hr^2, sum (sr - hr)^2, sum (lr - hr)^2} (double) for clips [B, T]  -> MSE / SNR
 *   mg_stft_frames    reflect-padded (center != 0), windowed frames [B * F, n_fft], F = mg_stft_num_frames(): the A
 *                     operand of the DFT, which the caller runs as the 1x1 case of mg_conv_fwd against a
 *                     [2 * (n_fft/2 + 1), n_fft] table of (cos, -sin) rows  (aF.spectrogram, util.py:170-171)
 *   mg_lsd_frames     per frame, from two interleaved (re, im) spectra [n_frames, 2 * n_bins]:
 *                     sqrt(mean_k (log10(|a_k|^2 + 1e-6) - log10(|b_k|^2 + 1e-6))^2)        (util.py:172-174) */
int mg_metrics_rows(const float* hr, const float* lr, const float* sr, int B, int T, double* out, void* stream);
int mg_stft_num_frames(int T, int n_fft, int hop, int center);
int mg_stft_frames(const float* x, int B, int T, const float* window, int n_fft, int hop, int center, float* frames,
                   void* stream);
int mg_lsd_frames(const float* spec_a, const float* spec_b, long long n_frames, int n_bins, float* out, void* stream);

/* The same metrics for MANY utterances in shared launches (the per-file compute_matrics of generate_audio.py:57-67 for a whole
 * test set).  mg_metric_row (a DEVICE array, one entry per utterance): sample t < len of row u is hr[hr_pos + t], lr[lr_pos + t],
 * sr[sr_pos + t] of three packed float32 buffers, each with its own total.  Windows are cut to their buffers (a sample that is
 * missing from one is skipped by the sums and enters a frame as 0), a row with len <= 0 is dead, there are no atomics and every
 * sum has one fixed order: a row has the same bits alone as inside any pack.  hr_shift [n_rows] or NULL: every hr sample of row u
 * enters as hr[p] + hr_shift[u], one float32 add (the operand mg_resample_rows forms from its shift).  No host synchronisation;
 * the launch count does not depend on n_rows.
 *   mg_metrics_rows_packed   out[u] = {sum hr^2, sum (sr - hr)^2, sum (lr - hr)^2} (double, mg_metrics_rows' arithmetic): chunks of
 *                            MG_MOMENTS_CHUNK samples counted from the row's first sample, each summed by one workgroup in a fixed
 *                            tree, then the chunks in ascending order.  max_len: the longest row (sizes the workspace and the grid;
 *                            longer rows lose their tail).  workspace: mg_metrics_rows_packed_workspace(n_rows, max_len) bytes.
 *                            A dead row gives {0, 0, 0}.
 *   mg_lsd_rows              out[frame_start[u] + f] = mg_lsd_frames' value for frame f of utterance u (float32), from the
 *                            waveforms: frames and spectra are never written.  frame_start [n_rows + 1] (device): the prefix sums
 *                            of mg_stft_num_frames(len_u, n_fft, hop, center), total_frames its last entry and the size of out.
 *                            Frames are reflected at the row's own [0, len) (center != 0; the host refuses n_fft / 2 >= len) and
 *                            multiplied by window [n_fft] as mg_stft_frames does; each spectrum is a real transform through an
 *                            n_fft / 2-point complex float32 Stockham FFT in LDS, the same statements for hr and sr (sr == hr
 *                            gives exactly 0).  n_fft 512, 1024 or 2048 (else MG_ERR_ARG), any hop >= 1. */
typedef struct { long long hr_pos, lr_pos, sr_pos, len; } mg_metric_row;
size_t mg_metrics_rows_packed_workspace(int n_rows, long long max_len);
int mg_metrics_rows_packed(const float* hr, long long hr_total, const float* lr, long long lr_total, const float* sr,
                           long long sr_total, const mg_metric_row* rows, int n_rows, long long max_len, const float* hr_shift,
                           double* out, void* workspace, size_t workspace_bytes, void* stream);
int mg_lsd_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                const long long* frame_start, long long total_frames, const float* hr_shift, const float* window, int n_fft,
                int hop, int center, float* out, void* stream);

/* The backward pass of mg_lsd_rows with respect to sr (hr is a constant), csrc/lsd_rows_grad.hip: with L_f the value mg_lsd_rows
 * stores for frame f of row u, grad_sr = d (sum_u sum_f grad_rows[u] L_f) / d sr.  The arguments up to `center` are mg_lsd_rows'
 * own and follow its rules.  grad_rows: float32 [n_rows], the gradient of row u's mean ALREADY divided by the row's frame count.
 * grad_sr: float32 [sr_total]; sample t < len of a live row is written once, at grad_sr[sr_pos + t], and nothing else is (the
 * caller zero-fills what it wants defined between the rows).  A frame with L_f == 0 (sr == hr, silence) contributes exactly 0,
 * where the formula has 0 / 0.  Two launches whatever n_rows is, no atomics, every sum in one fixed order: a row has the same
 * gradient bits alone as inside any pack.  workspace: mg_lsd_rows_backward_workspace(total_frames, n_fft) bytes, 16-byte aligned
 * (one window-weighted float32 gradient frame of n_fft samples per frame; 0: invalid arguments).  MG_ERR_ARG before any launch
 * for a null pointer (hr_shift may be NULL), n_fft outside {512, 1024, 2048}, a non-positive count, total or hop, a short or
 * misaligned workspace.  Precondition of a centred transform: len > n_fft / 2 (one reflection per end, what plan_metrics and
 * mg_stft_frames accept); a shorter live row is treated as dead here -- nothing of it is written. */
size_t mg_lsd_rows_backward_workspace(long long total_frames, int n_fft);
int mg_lsd_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                         int n_rows, const long long* frame_start, long long total_frames, const float* hr_shift,
                         const float* window, int n_fft, int hop, int center, const float* grad_rows, float* grad_sr,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The LSD of a dense training batch as a loss node of the step's convention (float32 [1] losses, constant factors in the node, the
 * upstream gradient read on the device); Python: metrics.lsd_loss_term.
 *   mg_lsd_mean_loss             loss[0] = float32(scale * (sum_f per_frame[f]) / total_frames) over mg_lsd_rows' per-frame array:
 *                                for equal-length clips the reference's .mean() (util/util.py:175).  One workgroup; the sum runs
 *                                in double, tiles of 256 consecutive frames in a fixed tree, then the tiles in ascending order,
 *                                rounded once: no atomics, bit-identical reruns, any total_frames >= 1.  per_frame is only read.
 *                                MG_ERR_ARG before the launch for a null pointer or total_frames <= 0.
 *   mg_lsd_rows_backward_seeded  mg_lsd_rows_backward -- its two launches, workspace, argument rules and guarantees -- with row u's
 *                                upstream gradient formed on the device instead of read from grad_rows: in double,
 *                                ((go[0] * scale) / n_rows) / frames_u with frames_u = frame_start[u + 1] - frame_start[u], rounded
 *                                to float32 once.  That is d (scale * mean_u mean_f L_f) / d sr times go[0] in the arithmetic
 *                                autograd performs around mg_lsd_rows_backward, so a power-of-two scale gives its bits.  go:
 *                                float32 [1] on the device, read when the kernel runs (a captured step follows a loss scale that
 *                                changes between replays); NULL is MG_ERR_ARG. */
int mg_lsd_mean_loss(const float* per_frame, long long total_frames, double scale, float* loss, void* stream);
int mg_lsd_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                                int n_rows, const long long* frame_start, long long total_frames, const float* hr_shift,
                                const float* window, int n_fft, int hop, int center, const float* go, double scale, float* grad_sr,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The multi-resolution STFT loss (spectral convergence + log-magnitude L1) of many utterances in shared launches,
 * csrc/stft_loss_rows.hip; Python: metrics.mrstft_many / mrstft_loss / mrstft_loss_term.  ONE resolution per call; the caller loops
 * over its resolutions on one stream.  hr, sr, rows, n_rows, frame_start, total_frames, n_fft, hop and center are mg_lsd_rows' own and
 * follow its rules (lr_pos of a row is not read; there is no hr_shift); window [n_fft] is the resolution's window (the Python side
 * passes the periodic Hann window, evaluated in float64 and rounded once).  With K = n_fft / 2 + 1, F_u the frames of row u, p = re^2
 * + im^2 of the float32 spectrum (the transform of the exact sample-times-window products runs in double and every bin is rounded
 * to float32 once, so the sign and clamp decisions below are float64's wherever two bins differ by more than float32 rounding; p
 * is formed in double) and m = sqrt(max(p, 1e-7)), everything after the spectrum in double:
 *     A_u = sum_{f,k} (m_hr - m_sr)^2,   B_u = sum_{f,k} m_hr^2,   C_u = sum_{f,k} |ln m_hr - ln m_sr|,
 *     loss_u = sqrt(A_u / B_u) + C_u / (F_u K).
 * Conventions at the non-smooth points: A_u == 0 makes the first term exactly 0, in value and gradient; a bin with ln m_hr ==
 * ln m_sr contributes 0 to the gradient (sign(0) = 0), and so does a bin with p_sr < 1e-7 (the clamp).  So sr == hr and silence
 * against silence give loss exactly 0 and gradient exactly 0, an all-zero sr a finite loss and gradient exactly 0.
 *   mg_stft_loss_rows   row_out[u] = {A_u, B_u, C_u, loss_u} (double [n_rows][4]; a dead row: four zeros).  Two launches whatever
 *                       n_rows is: every frame's three sums (a fixed tree over the frame's bins) into workspace, then each row's
 *                       frames in ascending order.  Frames and spectra are never written.  workspace:
 *                       mg_stft_loss_rows_workspace(total_frames) bytes (three doubles per frame; 0: invalid), 16-byte aligned.
 *   mg_stft_loss_rows_backward   grad_sr = d (sum_u grad_rows[u] loss_u) / d sr, hr constant.  row_sums: the row_out that
 *                       mg_stft_loss_rows wrote for the same operands and resolution (only read).  grad_rows: float32 [n_rows].
 *                       grad_sr: float32 [sr_total]; sample t < len of a live row is written once at grad_sr[sr_pos + t]
 *                       (accumulate == 0) or the rounded sum is added to what is there by the one thread that owns the sample
 *                       (accumulate != 0: the second and later resolutions, so that a multi-resolution gradient is the float32 sum
 *                       of the per-resolution ones in call order); nothing else is touched.  Two launches (the second is
 *                       mg_lsd_rows_backward's gather), no atomics, every sum in one fixed order.  workspace:
 *                       mg_stft_loss_rows_backward_workspace(total_frames, n_fft) bytes, 16-byte aligned (one float32 frame of
 *                       n_fft samples per frame).  A centred row with len <= n_fft / 2 is treated as dead, as in mg_lsd_rows_backward.
 *   mg_stft_loss_rows_backward_seeded   the same two launches for a loss node of the step's convention: every row's upstream
 *                       gradient is formed on the device, in double, as ((go[0] * scale) / n_rows) / n_res -- d (scale * mean_u
 *                       mean_r loss_{r,u}) times go[0].  go: float32 [1] on the device, read when the kernel runs (a captured
 *                       step follows a loss scale that changes between replays).  n_res: the number of resolutions of the mean.
 *   mg_stft_loss_mean   loss[0] = float32(scale * (sum_u (sum_r loss_{r,u}) / n_res) / n_rows) from row_out [n_res][n_rows][4] (the
 *                       row_out of n_res mg_stft_loss_rows calls, one after the other in one buffer): one workgroup, double, a
 *                       row's resolutions ascending, tiles of 256 rows in a fixed tree, the tiles ascending, rounded once.
 * A row has the same value and gradient bits alone as inside any pack.  No host synchronisation, static LDS only.  MG_ERR_ARG
 * before any launch for a null pointer, a non-positive count, total, hop or n_res, n_fft outside {512, 1024, 2048}, a short or
 * misaligned workspace. */
size_t mg_stft_loss_rows_workspace(long long total_frames);
int mg_stft_loss_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                      const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop, int center,
                      double* row_out, void* workspace, size_t workspace_bytes, void* stream);
size_t mg_stft_loss_rows_backward_workspace(long long total_frames, int n_fft);
int mg_stft_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                               int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft,
                               int hop, int center, const double* row_sums, const float* grad_rows, int accumulate, float* grad_sr,
                               void* workspace, size_t workspace_bytes, void* stream);
int mg_stft_loss_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total,
                                      const mg_metric_row* rows, int n_rows, const long long* frame_start, long long total_frames,
                                      const float* window, int n_fft, int hop, int center, const double* row_sums, const float* go,
                                      double scale, int n_res, int accumulate, float* grad_sr, void* workspace, size_t workspace_bytes,
                                      void* stream);
int mg_stft_loss_mean(const double* row_out, int n_rows, int n_res, double scale, float* loss, void* stream);

/* The multi-scale mel-spectrogram L1 loss of many utterances in shared launches, csrc/mel_loss_rows.hip; Python: metrics.mel_many /
 * mel_loss / mel_loss_term.  ONE resolution (n_fft, hop, n_mels) per call; the caller loops over its resolutions on one stream.  hr,
 * sr, rows, n_rows, frame_start, total_frames, window, n_fft, hop and center are mg_stft_loss_rows' own and follow its rules, and so
 * does everything up to the magnitudes: K = n_fft / 2 + 1 bins, p = re^2 + im^2 of the float32 spectrum (the transform runs in
 * double and every bin is rounded to float32 once; p is formed in double), m = sqrt(max(p, 1e-7)).  The filterbank operand:
 *   fbank   float32 [n_mels][K], dense (the Python side passes metrics.mel_fbank: HTK triangles without area normalisation,
 *           evaluated in float64 and rounded once); widened to double where it is read;
 *   band_k  int32 [n_mels][2]: filter j is non-zero on the bins [band_k[j][0], band_k[j][1]) only;
 *   band_j  int32 [K][2]: bin k lies in the filters [band_j[k][0], band_j[k][1]) only;
 *   n_mels  1 .. 256.
 * fbank is read inside those bands only and the kernels clip every band to the matrix: tables that do not agree with fbank lose
 * terms, nothing is read outside a buffer.  Per frame f and filter j, in double,
 *     E_j = sum_k fbank[j][k] m_k  (k ascending),   l_j = ln max(E_j, 1e-5),   loss_u = sum_{f,j} |l_hr - l_sr| / (F_u n_mels).
 * Conventions at the non-smooth points: a filter with l_hr == l_sr contributes 0 to the gradient (sign(0) = 0), and so do a filter
 * with E_sr <= 1e-5 (the floor of the logarithm) and a bin with p_sr < 1e-7 (the clamp).  So sr == hr and silence against silence
 * give loss exactly 0 and gradient exactly 0, an all-zero sr a finite loss and gradient exactly 0.
 *   mg_mel_loss_rows    row_out[u] = {sum_{f,j} |l_hr - l_sr|, 0, 0, loss_u} (double [n_rows][4], mg_stft_loss_rows' layout, so that
 *                       mg_stft_loss_mean over [n_res][n_rows][4] is the float32 loss of a dense batch; a dead row: four zeros).
 *                       Two launches whatever n_rows is: every frame's sum (a fixed tree over the frame's filters) into workspace,
 *                       then each row's frames in ascending order.  workspace: mg_mel_loss_rows_workspace(total_frames) bytes (one
 *                       double per frame; 0: invalid), 16-byte aligned.
 *   mg_mel_loss_rows_backward   grad_sr = d (sum_u grad_rows[u] loss_u) / d sr, hr constant: both spectra and both E again (nothing
 *                       is kept from the forward), dE_j = -grad_rows[u] sign(l_hr - l_sr) / (F_u n_mels E_sr), dm_k = sum_j
 *                       fbank[j][k] dE_j (j ascending), G_k = (dm_k / m_sr) X_sr[k], all in double; from G_k on
 *                       mg_stft_loss_rows_backward's float32 inverse, window product and gather, with its grad_rows, accumulate,
 *                       grad_sr and workspace (mg_mel_loss_rows_backward_workspace(total_frames, n_fft) bytes, 16-byte aligned).
 *   mg_mel_loss_rows_backward_seeded   the same two launches for a loss node of the step's convention: every row's upstream gradient
 *                       is formed on the device as float32(((go[0] * scale) / n_rows) / n_res), the quotient in double -- the row
 *                       gradient autograd hands the unseeded form for scale * mean_u mean_r loss_{r,u}.  go: float32 [1] on the
 *                       device, read when the kernel runs.
 * A row has the same value and gradient bits alone as inside any pack.  No host synchronisation, static LDS only, no atomics.
 * MG_ERR_ARG before any launch for a null or misaligned pointer, a non-positive count, total, hop or n_res, n_fft outside {512, 1024,
 * 2048}, n_mels outside 1 .. 256, a short or misaligned workspace. */
size_t mg_mel_loss_rows_workspace(long long total_frames);
int mg_mel_loss_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                     const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop, int center,
                     const float* fbank, const int* band_k, const int* band_j, int n_mels, double* row_out, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t mg_mel_loss_rows_backward_workspace(long long total_frames, int n_fft);
int mg_mel_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                              int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft,
                              int hop, int center, const float* fbank, const int* band_k, const int* band_j, int n_mels,
                              const float* grad_rows, int accumulate, float* grad_sr, void* workspace, size_t workspace_bytes,
                              void* stream);
int mg_mel_loss_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total,
                                     const mg_metric_row* rows, int n_rows, const long long* frame_start, long long total_frames,
                                     const float* window, int n_fft, int hop, int center, const float* fbank, const int* band_k,
                                     const int* band_j, int n_mels, const float* go, double scale, int n_res, int accumulate,
                                     float* grad_sr, void* workspace, size_t workspace_bytes, void* stream);

/* Segment stitching of generate_audio.py:40-53: seg [n_seg, seg_len] (the [n_seg,1,1,T] inference outputs) -> one
 * waveform of mg_stitch_length() samples (-1: invalid arguments; 2*overlap must be < seg_len).  overlap == 0
 * concatenates; overlap > 0 halves the first/last `overlap` samples of every segment, overlap-adds at stride
 * seg_len - overlap (F.fold) and crops `overlap` samples from both ends.  float32, or float64 when is_f64. */
long long mg_stitch_length(int n_seg, int seg_len, int overlap);
int mg_stitch_segments(const void* seg, int n_seg, int seg_len, int overlap, void* out, int is_f64, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generic-geometry transform and the remaining codec branches (csrc/codec_generic.hip): MDCT4 / IMDCT4 for any
 * win_length <= n_fft, hop_length <= win_length (models/mdct.py:365-489; the dense cosine contraction itself runs as the 1x1
 * case of mg_conv_fwd), and Audio2MDCT.normalize / denormalize (models/pix2pixHD_model.py:83-137) in every mode.
 * ------------------------------------------------------------------------------------------ */
#define MG_CODEC_DB 3        /* 20 log10(max(|X| + min_value, min_value)) - 20  (torchaudio amplitude_to_DB, unpinned) */
#define MG_CODEC_EXPLICIT 4  /* --explicit_encoding: two dB channels of alpha-mixed positive / negative parts */
/* frames[b, f, k] = fl32(x[b, f*hop + k - start_pad] * window[k]), zero outside [0, T)   (mdct.py:393-410) */
int mg_frames_window(const float* x, int B, int T, int win, int hop, int start_pad, int F, const float* window,
                     float* frames, void* stream);
/* X [B][n] raw coefficients -> out [B][C][n] (C = 2 for MG_CODEC_EXPLICIT, else 1), optional pair [B][n][2] =
 * (v, 2|v| + nr0) (C == 1), per_sample: min/max per (b, channel) into min_out / max_out [B*C] (scratch_u32: 2*B*C words),
 * stats: double[2] = sum, sum of squares of the pre-normalisation values. */
int mg_codec_forward(const float* X, int B, int n, int mode, float gain, float alpha, float min_value, float nr0, float nr1,
                     float src_min, float src_max, int per_sample, float* out, float* pair, float* min_out, float* max_out,
                     void* scratch_u32, double* stats, void* stream);
/* spec [B][C][n] -> X [B][n]; min_b / max_b [B*C] or both null (src_min / src_max) */
int mg_codec_inverse(const float* spec, int B, int n, int mode, float gain, float alpha, float min_value, float nr0, float nr1,
                     float src_min, float src_max, const float* min_b, const float* max_b, float* X, void* stream);
/* Backward of the RAW / ARCSINH / RANGE codec on [B][n] (dX/ds as for mg_imdct4_backward; min_b / max_b [B] or (src_min, src_max)):
 * to_spectro == 0: out = scale * grad * dX/ds(spec)   (to_audio's backward; scale = 4/n_fft after the framed contraction)
 * to_spectro != 0: out = scale * grad / dX/ds(spec)   (to_spectro's backward).  spec may be NULL for RAW. */
int mg_codec_backward(const float* grad, const float* spec, int B, int n, int mode, int to_spectro, float scale, float gain,
                      float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b, float* out,
                      void* stream);
/* out[b, t] = 4/n_fft * sum_f window[k] * Y[b, f, k], k = t + crop - f*hop   (mdct.py:469-486), float32 or float64 out */
int mg_overlap_add(const float* Y, int B, int F, int win, int hop, int n_fft, const float* window, int crop, void* out,
                   int out_len, int is_f64, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3/K4/K6  Implicit-GEMM convolution on the f32 MFMA pipe (exact float32).
 *   Replaces nn.Conv2d / nn.ConvTranspose2d / nn.ReflectionPad2d forward and backward at
 *   models/networks.py:207-210, 308-309, 329, 349-352, 387-392, 406-411, 440, 456, 649-670.
 *
 *   The geometry always describes the *convolution* (for ConvTranspose2d: the convolution whose
 *   data-gradient it is): x [B, H, W, Ci] --(KHxKW, stride, pad, zero|reflect)--> y [B, OH, OW, Co].
 */
typedef struct {
    int B, H, W, Ci;
    int OH, OW, Co;
    int KH, KW, stride, pad;
    int reflect; /* 0: zero padding, 1: reflection padding (ReflectionPad2d(pad) folded into the gather) */
    int precision; /* MG_PRECISION_F32: exact float32 on the f32 MFMA pipe.  MG_PRECISION_F16: the arithmetic of
                    * torch.autocast(float16) for convolutions (train.py:161-164 with --fp16): operands rounded to
                    * float16 as they are staged, products on the f16 MFMA pipe, float32 accumulation, outputs of the
                    * forward / data-gradient passes rounded through float16 (overflow -> inf, as a float16 tensor
                    * would), weight gradients kept in float32.  Tensors stay float32 in memory.
                    * MG_PRECISION_F32_WINO43 (opt-in, forward passes of inference only): exact float32 products as
                    * MG_PRECISION_F32, in Winograd F(4x4,3x3) arithmetic where the layer is eligible -- 3x3 stride-1 pad-1,
                    * H and W multiples of 4, Ci and Co multiples of 16 and >= 256 (MG_WINO43_MIN_C in the environment, read
                    * per call, overrides the 256).  36 positions, K = Ci, T = B*(H/4)*(W/4) tiles; points (0, 1, -1, 1/2, -2,
                    * inf), error ~3.5e-6 of the output scale at Ci = 1024 (F(2x2,3x3): 4e-7).  An ineligible geometry runs
                    * exactly as under MG_PRECISION_F32 (same kernels, same bits).  An eligible one has no gradients: the
                    * data- and weight-gradient entry points return MG_ERR_UNSUPPORTED and their workspace queries 0.
                    * MG_PRECISION_F16_INFER (opt-in, forward passes of inference only): the arithmetic of MG_PRECISION_F16
                    * -- operands rounded to float16, exact products on the f16 MFMA, float32 accumulation, convolution
                    * outputs rounded through float16, tensors float32 in memory -- with the Winograd F(2x2,3x3) images of an
                    * eligible layer kept as float16 in HBM (csrc/wino_h16.h): 3x3 stride-1 pad-1, H and W even, Ci and Co
                    * multiples of 64 and >= 256, >= 256 tiles (MG_INFER_F16_MIN_C / MG_INFER_F16_MIN_TILES in the
                    * environment, read per call, override the two 256), and not one of the weight-streaming layers of small
                    * batches (<= 2 Co pixels), which keep their float16 GEMM path unless MG_INFER_F16_MIN_TILES is set.  An ineligible geometry runs exactly as
                    * under MG_PRECISION_F16 (same kernels, same bits).  An eligible one has no gradients: the data- and
                    * weight-gradient entry points return MG_ERR_UNSUPPORTED and their workspace queries 0; its u / v images
                    * (mg_wino_tiles) are float16: 16*Co*Ci and 16*T*Ci halves, sized by the same two queries. */
} mg_conv_geom;
#define MG_PRECISION_F32 0
#define MG_PRECISION_F16 1
#define MG_PRECISION_F32_WINO43 2
#define MG_PRECISION_F16_INFER 3
/* the two values whose arithmetic is half precision */
#define MG_PRECISION_IS_HALF(p) ((p) == MG_PRECISION_F16 || (p) == MG_PRECISION_F16_INFER)

/* y = act(conv(x, w) + bias)            (bias nullable).  workspace (nullable): mg_conv_fwd_workspace() bytes of
 * scratch that lets deep-K / small-M*N layers split K across workgroups (without it they run unsplit). */
int mg_conv_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act,
                void* workspace, size_t workspace_bytes, void* stream);
size_t mg_conv_fwd_workspace(const mg_conv_geom* g);
/* dx = conv^T(dy, w) (+ bias, act)      data gradient of the convolution == ConvTranspose2d forward */
int mg_conv_dgrad(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t mg_conv_dgrad_workspace(const mg_conv_geom* g);
/* Layers with channel counts that are multiples of 16 run as batched GEMMs over Winograd-transformed operands:
 *   3x3 stride-1 pad-1 (ResnetBlock)            F(2x2,3x3), P = 16 positions, K = Ci,   T = B*(H/2)*(W/2) tiles (H, W even)
 *   4x4 stride-1 pad-2 (PatchGAN, H and W odd)  F(2x2,4x4), P = 25,           K = Ci,   T = B*((H+1)/2)*((W+1)/2)
 *   4x4 stride-2 pad-2 (PatchGAN, large only)   F(4x4,2x2) over the space-to-depth view, P = 25, K = 4*Ci,
 *                                               T = B*ceil(OH/4)*ceil(OW/4)
 * A training step runs forward, data gradient and weight gradient of a layer with the
 * same weights / activations / output gradient, so the caller may hold the transformed images and hand them to the _w
 * entry points (every pointer optional; NULL = transform internally, which is what the plain entry points do):
 *   u   U = G w G^T            P*Co*K floats   mg_conv_wino_prepare() fills it; read by fwd and dgrad
 *   v   V = B^T x B            P*T*K floats    WRITTEN by mg_conv_fwd_w, read by mg_conv_wgrad_w
 *   md  Md = A dy A^T          P*T*Co floats   WRITTEN by mg_conv_dgrad_w, read by mg_conv_wgrad_w
 * Sizes (never computed by the caller): mg_conv_wino_weights_bytes() and mg_conv_wino_tiles_bytes(g, 0 = v | 1 = md); 0 means
 * "this geometry / configuration does not use that image" and the pointer must stay NULL.  Every image must come
 * from the tensors passed in the same step. */
typedef struct {
    const float* u;
    float* v;
    float* md;
    const float* add;   /* mg_conv_dgrad_w only, any geometry: dx += add ([B,H,W,Ci]) -- the gradient a skip connection brings to
                         * the same tensor (ResnetBlock, models/networks.py:462), folded into the call's last kernel where the path
                         * allows and added by a separate pass otherwise; NULL for every other call */
    unsigned flags;     /* MG_TILES_*_FILLED (MG_PRECISION_F16 layers whose tiles are plain float16 copies): the copy is already in
                         * the buffer -- written by the kernel that produced x / dy (mg_instnorm_fwd_h, mg_instnorm_bwd_h,
                         * mg_conv_fwd_instnorm_h) -- so the call skips its own cast pass.  Paths that do not use the copy ignore it. */
} mg_wino_tiles;
#define MG_TILES_V_FILLED 1u    /* mg_conv_fwd_w: v holds float16(x) (MG_PRECISION_F16 implicit GEMMs) / B^T x B written by
                                   mg_conv_fwd_instnorm_next of the layer in front (float32 F(2x2,3x3) layers) */
#define MG_TILES_MD_FILLED 2u   /* mg_conv_dgrad_w: md holds float16(dy) */
size_t mg_conv_wino_weights_bytes(const mg_conv_geom* g);
size_t mg_conv_wino_tiles_bytes(const mg_conv_geom* g, int which);
int mg_conv_wino_prepare(const mg_conv_geom* g, const float* w, float* u, void* stream);
/* What a caller that holds these images across the passes of a step has to know about a layer, in one query: every field follows
 * from the geometry and the environment of the moment, as the launches do.  (The struct carries a tag, not a typedef, so that it
 * can share its name with the function: write `struct mg_conv_traits`.)  MG_ERR_ARG: out is NULL or the geometry is invalid. */
#define MG_IMAGE_NONE 0       /* mg_conv_wino_weights_bytes(g) == 0: the layer keeps no weight image */
#define MG_IMAGE_WINO_F32 1   /* U = G w G^T in float32 */
#define MG_IMAGE_WINO_F16 2   /* ... in float16 (MG_PRECISION_F16_INFER layers on float16 images) */
#define MG_IMAGE_CAST 3       /* the plain float16 copy of the OHWI weights (the float16 GEMM paths of MG_PRECISION_F16) */
#define MG_IMAGE_CO1 4        /* the weights of a single-output-channel layer padded to 64 tap rows, float32 */
struct mg_conv_traits {
    int weight_image;         /* MG_IMAGE_*: what mg_conv_wino_prepare writes into u */
    int weight_positions;     /* P of a Winograd image (16, 25 or 36), 0 for the other kinds */
    int weight_elem;          /* bytes per element of u (0 for MG_IMAGE_NONE) */
    int images_half;          /* the layer's Winograd images u, v and a handed-over v_next are float16 (MG_IMAGE_WINO_F16) */
    int tiles;                /* 0: v / md are absent, or Winograd images, which the weight gradient takes only as a pair;
                               * 1: they are the float16 copies of x / dy, each usable without the other;
                               * 2: md is the scattered dy of a single-output-channel layer (usable alone; v: its rounded x) */
    int precast[2];           /* [0]: mg_conv_fwd_w honours MG_TILES_V_FILLED with v = float16(x) written by x's producer;
                               * [1]: mg_conv_dgrad_w honours MG_TILES_MD_FILLED with md = float16(dy) */
    int vnext_positions;      /* != 0 where mg_conv_wino_vnext_ok(g): the positions of the family v_next is written for (an image
                               * is only good for a layer of the same family and element type) */
    int md_from_norm;         /* mg_conv_wino_md_from_norm_ok(g) */
    int wgrad_adam;           /* mg_conv_wgrad_adam_ok(g) */
    int wgrad_checks_finite;  /* mg_conv_wgrad_checks_finite(g) */
    int wgrad_h16;            /* mg_conv_wgrad_h16_ok(g) */
};
int mg_conv_traits(const mg_conv_geom* g, struct mg_conv_traits* out);
int mg_conv_fwd_w(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act,
                  void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles);
/* y_raw = conv(x, w) + bias (mg_conv_fwd_w with no activation) followed by mg_instnorm_fwd(y_raw) -> y = act((y_raw - mean)
 * * rstd) + residual, mean / rstd [B][Co]: the [conv3x3, InstanceNorm2d(affine=False), ReLU] / [conv3x3, InstanceNorm2d, + x]
 * pairs of ResnetBlock (models/networks.py:440-462).  When the layer runs as Winograd F(2x2,3x3) and a sample's map is
 * <= 640 pixels, the inverse transform, the statistics and the normalisation are ONE kernel; otherwise the two calls are
 * made back to back -- same results either way (statistics in double, fixed reduction order).  y_raw is kept because the
 * InstanceNorm backward recomputes the normalised value from it; y_raw = NULL (inference) skips that store (the two-call path
 * then normalises in place).  workspace >= mg_conv_fwd_instnorm_workspace(g). */
size_t mg_conv_fwd_instnorm_workspace(const mg_conv_geom* g);
int mg_conv_fwd_instnorm_w(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                           int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                           size_t workspace_bytes, void* stream, const mg_wino_tiles* wt);
/* The backward mirror: for a layer with mg_conv_wino_md_from_norm_ok(g) != 0, mg_instnorm_bwd_wino_md turns the gradient gy at
 * the InstanceNorm output (y_raw, mean, rstd, act as saved by mg_conv_fwd_instnorm_w) straight into md = A dy A^T, the
 * Winograd image of the gradient at the convolution output (mg_conv_wino_tiles_bytes(g, 1) bytes) -- InstanceNorm backward
 * and the data gradient's first transform in one kernel; dy itself is never written.  mg_conv_dgrad_w(g, dy = NULL, ...,
 * wt->md = md) and mg_conv_wgrad_w(g, x = NULL, dy = NULL, ..., dbias = NULL, wt->v, wt->md) then start from the images. */
int mg_conv_wino_md_from_norm_ok(const mg_conv_geom* g);
int mg_instnorm_bwd_wino_md(const mg_conv_geom* g, const float* gy, const float* y_raw, const float* mean, const float* rstd,
                            int act, float* md, void* stream);
/* mg_conv_fwd_instnorm_w that also writes float16(y) (y16: B*OH*OW*Co halves, 8-byte aligned; NULL = none) for the next
 * MG_PRECISION_F16 layer's MG_TILES_V_FILLED.  MG_PRECISION_F16 geometries only (MG_ERR_UNSUPPORTED otherwise). */
int mg_conv_fwd_instnorm_h(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                           int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                           size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles, void* y16);
/* mg_conv_fwd_instnorm_w that ALSO writes v_next = B^T y B, the Winograd input image of its own output y for a following 3x3
 * stride-1 pad-1 convolution over the same map (next_reflect: that layer's padding mode): ResnetBlock chains conv -> InstanceNorm ->
 * conv (models/networks.py:440-462), and the workgroup that normalises a slab of y holds exactly the pixels the next layer's
 * tiles need.  v_next: mg_conv_wino_tiles_bytes(g_next, 0) bytes (16 * T * Co floats); the next layer's call takes it as tiles->v
 * with MG_TILES_V_FILLED and skips its own input transform -- bit-identical results (the same float32 arithmetic on the same
 * values).  Only where mg_conv_wino_vnext_ok(g) != 0 (float32 F(2x2,3x3) layers on maps of <= 64 tiles per sample); MG_ERR_ARG
 * elsewhere.  Replaces nothing in the reference: it removes one launch and one read of y per trunk layer.
 * MG_PRECISION_F32_WINO43 layers that run as F(4x4,3x3) have the same pair: on maps of <= 40 tiles (640 pixels) per sample with
 * Co % 32 == 0 the inverse transform and the InstanceNorm are one kernel, mg_conv_wino_vnext_ok(g) != 0, and v_next is the
 * 36 * T * Co float image of a following F(4x4,3x3) layer.  The caller hands an image only to a layer of the family it was written
 * for (the same mg_conv_traits.vnext_positions). */
int mg_conv_wino_vnext_ok(const mg_conv_geom* g);
int mg_conv_fwd_instnorm_next(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                              int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                              size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles, float* v_next, int next_reflect);
/* The MG_PRECISION_F16_INFER sibling of the two calls above, for a layer that runs on float16 Winograd images
 * (mg_conv_wino_vnext_ok(g) != 0 under that precision: maps of <= 64 tiles per sample; MG_ERR_ARG elsewhere).  v_next16 (nullable):
 * float16(B^T y B), 16 * T * Co halves = mg_conv_wino_tiles_bytes(g_next, 0) bytes, which the next layer takes as tiles->v with
 * MG_TILES_V_FILLED.  y16 (nullable): float16(y), as mg_conv_fwd_instnorm_h writes it, for a consumer that stages its operand from
 * a plain float16 copy.  The convolution output is rounded through float16 before the statistics; y is float32. */
int mg_conv_fwd_instnorm_next_h(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                                int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                                size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles, void* v_next16, int next_reflect,
                                void* y16);
int mg_conv_dgrad_w(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                    void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles);
/* dw [Co, KH, KW, Ci] = sum over pixels; dbias [Co] (nullable) = column sums of dy.
 * accumulate != 0 adds into dw / dbias instead of overwriting.  workspace: mg_conv_wgrad_workspace() bytes. */
int mg_conv_wgrad(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t mg_conv_wgrad_workspace(const mg_conv_geom* g);
int mg_conv_wgrad_w(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                    void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles);
/* --fp16 (train.py:183-199, torch.cuda.amp.GradScaler.unscale_'s inf / nan check): where mg_conv_wgrad_checks_finite(g) != 0 the
 * weight-gradient kernel inspects its own results -- mg_conv_wgrad_chk stores 1.0f to *found_inf (device memory; left alone
 * otherwise) when an element of dw, after accumulation, is inf or nan, so the caller can leave dw out of its mg_scaler_check
 * pass (the 2048-channel trunk layers of configs[2] / [3]: 151 MB each).  found_inf = NULL: same as mg_conv_wgrad_w.
 * found_inf != NULL on a geometry without the check: MG_ERR_UNSUPPORTED. */
int mg_conv_wgrad_checks_finite(const mg_conv_geom* g);
int mg_conv_wgrad_chk(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles, float* found_inf);
/* Round 6: the same weight gradient STORED as float16 (dw16: Co * KH * KW * Ci halves, OHWI) -- the dtype an autocast layer's
 * weight gradient has in the reference (train.py:161-164).  Only where mg_conv_wgrad_h16_ok(g) != 0 (the short-reduction GEMM
 * of the weight-streaming trunk layers, whose 151 MB float32 output stream is what bounds it); found_inf (nullable) as above,
 * with float16's overflow criterion; accumulate adds into the float16 values.  No bias gradient (those layers' biases feed an
 * InstanceNorm: identically zero). */
int mg_conv_wgrad_h16_ok(const mg_conv_geom* g);
int mg_conv_wgrad_h16(const mg_conv_geom* g, const float* x, const float* dy, void* dw16, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream, float* found_inf);
/* Round 3 (single process, float32): the weight side of a Winograd F(2x2,3x3) layer in one pass.  Instead of writing dw,
 * the call applies torch.optim.Adam's update (pix2pixHD_model.py:350-351) to (w, m, v) straight from the Winograd-domain
 * gradient and leaves u = G w G^T of the UPDATED weights (mg_conv_wino_weights_bytes(g) bytes) for the next forward:
 * the gradient never exists in HBM, the weights make one round trip instead of three.  state: the optimiser's device
 * clock double[6] = {step, lr, lr / (1 - b1^step), sqrt(1 - b2^step), 1 - b1^(step+1), sqrt(1 - b2^(step+1))} BEFORE this
 * iteration's mg_adam_tick (the call reads [1], [4], [5]; mg_adam_tick / mg_adam_tick_amp maintain them, mg_adam_prime
 * initialises [4], [5] for a fresh or restored clock).  Same results as mg_conv_wgrad_w + mg_adam_step_dev +
 * mg_conv_wino_prepare, bit for bit.  The caller guarantees what the fusion assumes: one optimiser step per backward
 * pass, no other contribution to this weight's gradient, no gradient reduction across processes, no loss scaling. */
typedef struct {
    float* m;
    float* v;
    float* u;
    const double* state;
    float beta1, beta2, eps, grad_scale;
} mg_wino_adam;
int mg_conv_wgrad_adam_ok(const mg_conv_geom* g);
int mg_conv_wgrad_adam_w(const mg_conv_geom* g, const float* x, const float* dy, float* w, const mg_wino_adam* adam,
                         void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* tiles);
/* Name of the kernel instance a pass (0 fwd, 1 dgrad, 2 wgrad) launches for this geometry -- the symbol
 * rocprofv3 reports -- so bench.py can attribute event-timed launches per kernel.  out: host buffer >= 64 B. */
int mg_conv_plan_name(int pass, const mg_conv_geom* g, char* out, int out_len);
/* K splits of that launch where the pass takes the LDS-DMA implicit-GEMM kernels (conv_{fwd,dgrad,wgrad}_dma_kernel; 1 = unsplit)
 * or is a Winograd layer (the splits of its batched Winograd-domain GEMM), 0 for every other kernel family: lets a host-only
 * test pin the planner (workgroups = tiles x splits). */
int mg_conv_plan_splits(int pass, const mg_conv_geom* g);
/* Launch order of that kernel where the pass takes the LDS-DMA forward / data-gradient kernels, under the current environment:
 * gm = row tiles per group of the tile order (0 = row tiles fastest over the whole split), cls_order = the stride-2 data
 * gradient's parity-class order (1 = light and heavy classes paired, 0 = heaviest first; MG_DGRAD_CLASS_ORDER=0|1 forces one).
 * Both 0 for every other pass and family. */
int mg_conv_plan_order(int pass, const mg_conv_geom* g, int* gm, int* cls_order);
/* FLOPs issued by that kernel for this geometry (direct: 2*MACs; Winograd layers: the P batched GEMMs, 2*P*T*Co*K). */
double mg_conv_plan_flops(int pass, const mg_conv_geom* g);
/* One-shot timing probe for bench.py: the next mg_conv_{fwd,dgrad,wgrad} call records hipEvent e0 / e1 on its launch
 * stream immediately around its main GEMM kernel (not around transforms / split-K epilogues), then disarms. */
void mg_probe_arm(void* e0, void* e1);
/* column sums: out[c] (+)= sum_m a[m, c]  -- bias gradients of ConvTranspose2d layers */
int mg_colsum(const float* a, long long M, int C, float* out, int accumulate, void* workspace,
              size_t workspace_bytes, void* stream);
size_t mg_colsum_workspace(long long M, int C);

/* ------------------------------------------------------------------------------------------
 * K5  InstanceNorm2d(affine=False, eps) with fused activation / residual (networks.py:26, 306,
 *     462, 650-666).  x, y: [B, HW, C].  mean / rstd: [B, C] (saved for backward).
 *     y = act((x - mean) * rstd) (+ residual).
 */
int mg_instnorm_fwd(const float* x, int B, int HW, int C, float eps, int act, const float* residual, float* y,
                    float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream);
/* dx from dy (gradient wrt y, excluding the residual branch), the saved x, mean, rstd. */
int mg_instnorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                    int act, float* dx, void* workspace, size_t workspace_bytes, void* stream);
size_t mg_instnorm_workspace(int B, int HW, int C);
/* --fp16 (train.py:161-164): the same two calls, additionally writing the float16 copy of their output (y16 / dx16: B*HW*C
 * halves, 8-byte aligned, C % 4 == 0; NULL = none) -- the operand staging the next autocast convolution would otherwise do in
 * a cast pass of its own (hand it over with MG_TILES_V_FILLED / MG_TILES_MD_FILLED).  The float32 results are unchanged. */
int mg_instnorm_fwd_h(const float* x, int B, int HW, int C, float eps, int act, const float* residual, float* y,
                      float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream, void* y16);
int mg_instnorm_bwd_h(const float* dy, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                      int act, float* dx, void* workspace, size_t workspace_bytes, void* stream, void* dx16);
/* Round 6: the same passes with a SECOND gradient of the tensor (dy2, nullable): the kernels read dy + dy2 (one float32 addition per
 * element, exactly autograd's accumulation add) -- a discriminator feature map has two consumers, the next layer and the
 * feature-matching loss (pix2pixHD_model.py:443-451), and the loss's gradient joins the layer's here instead of in an add launch. */
int mg_instnorm_bwd_add(const float* dy, const float* dy2, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                        int act, float* dx, void* workspace, size_t workspace_bytes, void* stream, void* dx16);

/* ------------------------------------------------------------------------------------------
 * K10  bottleneck-transformer block pieces (bottleneck_transformer_pytorch==0.1.4 BottleStack, call sites
 *      models/networks.py:232-235, 341-344; third-party, parity unpinned).  The block's 1x1 convolutions use
 *      mg_conv_*.
 *  BatchNorm2d over R = B*H*W rows of an NHWC tensor [R, C]:
 *      training: batch statistics (biased var for normalisation, unbiased into running_var, momentum m);
 *      eval: running statistics.  y = act(gamma * xhat + beta + residual)  (act in {NONE, RELU}; residual nullable).
 */
/*  Round 3: statistics and application are separate launches with per-slice double-precision partial sums
 *  [mg_batchnorm_slices()][2][C] between them (mg_batchnorm_workspace(C) bytes): sums -> (a data-parallel run may
 *  all-reduce the partials here: SyncBN, then count = rows of the whole batch) -> apply.
 *      mg_batchnorm_sums      partials of (sum x, sum x^2)
 *      mg_batchnorm_fwd       training: statistics from `sums` / `count`;  eval: running statistics (sums may be NULL)
 *      mg_batchnorm_bwd_sums  partials of (sum g, sum g * xhat), g = dy masked by the ReLU of y
 *      mg_batchnorm_bwd       dgamma / dbeta from local_sums (this rank's samples), dx from batch_sums / count */
size_t mg_batchnorm_workspace(int C);
int mg_batchnorm_slices(void);
int mg_batchnorm_sums(const float* x, int R, int C, void* sums, void* stream);
int mg_batchnorm_fwd(const float* x, int R, int C, float eps, float momentum, int training, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, const float* residual, int act,
                     float* y, float* save_mean, float* save_rstd, const void* sums, double count, void* stream);
int mg_batchnorm_bwd_sums(const float* dy, const float* x, const float* y, int R, int C, const float* mean,
                          const float* rstd, int act, void* sums, void* stream);
int mg_batchnorm_bwd(const float* dy, const float* x, const float* y, int R, int C, const float* gamma,
                     const float* mean, const float* rstd, int act, int training, float* dx, float* dresidual,
                     float* dgamma, float* dbeta, int accumulate, const void* local_sums, const void* batch_sums,
                     double count, void* stream);
/*  Multi-head self attention with absolute position embeddings (rel_pos_emb=False):
 *      qkv [B, fh*fw, 3*heads*d] (channel = which*heads*d + head*d + dd), emb_h [fh, d], emb_w [fw, d];
 *      sim = (q * d^-0.5) (k + emb_h[y] + emb_w[x])^T, out [B, fh*fw, heads*d] = softmax(sim) v.
 *      P [B, heads, n, n] receives the probabilities (saved for backward).  fh*fw <= 256, d <= 128 (more than 128 tokens
 *      run on the MFMA-tiled family of bot_attn.hip; larger maps are MG_ERR_ARG).
 *      Forward and backward both need B, fh, fw, heads and d >= 1 and return MG_ERR_ARG otherwise, before any launch.
 *      Backward: demb_h / demb_w may both be NULL (no table gradient); accumulate = 1 adds into them. */
int mg_attention_fwd(const float* qkv, const float* emb_h, const float* emb_w, int B, int fh, int fw, int heads, int d,
                     float* out, float* P, void* stream);
int mg_attention_bwd(const float* qkv, const float* emb_h, const float* emb_w, const float* dout, const float* P, int B,
                     int fh, int fw, int heads, int d, float* dqkv, float* demb_h, float* demb_w, int accumulate,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t mg_attention_bwd_workspace(int B, int fh, int fw, int heads, int d);

/* K7  elementwise activation backward for conv epilogues: dx = dy * act'(y)  (in place allowed) */
int mg_act_bwd(const float* dy, const float* y, float* dx, long long n, int act, void* stream);
int mg_act_bwd_add(const float* dy, const float* dy2, const float* y, float* dx, long long n, int act, void* stream);
/* out = a + b (residual joins outside a norm), in place allowed */
int mg_add(const float* a, const float* b, float* out, long long n, void* stream);

/* K8  AvgPool2d(3, stride 2, padding 1, count_include_pad=False) (networks.py:249-250, 525-526) */
int mg_avgpool3s2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream);
int mg_avgpool3s2_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream);
/* K9  nearest x2 upsample (networks.py:396) */
int mg_upsample2x_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream);
int mg_upsample2x_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream);

/* discriminator input assembly (pix2pixHD_model.py:420-424, 439-440):
 *   out [B, HW, 3] = (lr, s, 2|s| + nr0);  backward: ds = g1 + 2*sign(s)*g2 */
int mg_dinput_fwd(const float* lr, const float* s, long long n, float nr0, float* out, void* stream);
/* ... and without --abs_spectro --arcsinh_transform (pix2pixHD_model.py:425-427, 440 else branch): the plain
 *   torch.cat((a, b), dim=1) of NHWC tensors, n pixels of Ca / Cb channels, and its backward (ga / gb nullable) */
int mg_cat2_fwd(const float* a, int Ca, const float* b, int Cb, long long n, float* out, void* stream);
int mg_cat2_bwd(const float* g, int Ca, int Cb, long long n, float* ga, float* gb, void* stream);
int mg_dinput_bwd(const float* dout, const float* s, long long n, float* ds, void* stream);
/* generator input pair [n, 2] = (s, 2|s| + nr0) from a spectrogram (pix2pixHD_model.py:400-402) */
int mg_pair_fwd(const float* s, long long n, float nr0, float* out, void* stream);
/* mean_std[0] = stats[0] / n, mean_std[1] = sqrt(max(0, (stats[1] - stats[0]^2 / n) / (n - 1))) -- the `mean` / `std` entries of
 * to_spectro's norm_param (models/pix2pixHD_model.py:108-109: log_spectro.mean(), log_spectro.var().sqrt()) from the {sum, sum of
 * squares} K1 accumulates, in float64 like the torch expression it replaces. */
int mg_stats_finalize(const double* stats, long long n, float* mean_std, void* stream);

/* ------------------------------------------------------------------------------------------
 * K11  losses (networks.py:127-137 GANLoss/LSGAN, pix2pixHD_model.py:443-451 feature matching).
 *   fwd: loss[0] (+)= scale * mean((pred - target)^2)   |   scale * mean(|a - b|)
 *        (two-stage fixed-order reduction in double: deterministic; workspace >= mg_loss_workspace()).
 *   bwd: grad = d loss / d pred (resp. a) * grad_out[0]  (grad_out: device scalar, nullable == 1).
 *   Each of these single-tensor calls is mg_loss_multi_{fwd,bwd} below on a list of one item (the same kernels, the same bits);
 *   one item has at most 1024 partials, so mg_loss_workspace() bytes serve it.
 */
size_t mg_loss_workspace(void);
int mg_mse_const_fwd(const float* pred, long long n, float target, float scale, float* loss, int accumulate,
                     void* workspace, void* stream);
int mg_mse_const_bwd(const float* pred, long long n, float target, float scale, const float* grad_out, float* grad,
                     void* stream);
/* --no_lsgan (networks.py:106-109, 676-677): nn.BCELoss against a constant label on probabilities (log terms clamped at -100,
 * gradient (p - t) / max((1 - p) p, 1e-12) -- torch's rules), and the nn.Sigmoid that produces them. */
int mg_bce_const_fwd(const float* pred, long long n, float target, float scale, float* loss, int accumulate,
                     void* workspace, void* stream);
int mg_bce_const_bwd(const float* pred, long long n, float target, float scale, const float* grad_out, float* grad,
                     void* stream);
int mg_sigmoid_fwd(const float* x, float* y, long long n, void* stream);
int mg_sigmoid_bwd(const float* dy, const float* y, float* dx, long long n, void* stream);
int mg_l1_fwd(const float* a, const float* b, long long n, float scale, float* loss, int accumulate, void* workspace,
              void* stream);
int mg_l1_bwd(const float* a, const float* b, long long n, float scale, const float* grad_out, float* grad_a,
              void* stream);
/* The same three losses over a LIST of tensors, one launch per stage (kind 0: mean((a - target)^2), 1: mean(|a - b|), 2: BCE against
 * the constant label `target`): loss (+)= sum_i scale * loss_i -- the feature-matching sum over the discriminators' intermediate
 * layers (models/pix2pixHD_model.py:440-449) and the per-scale GAN terms.  Bit-identical to the accumulate-in-place sequence of
 * one-item calls in list order (every item keeps the partial blocks and the grid stride it has alone).
 * Backward: grad[i][0..n) = d(scale * loss_i)/da_i * grad_out[0]; additionally grad[i][n .. n + zero_tail) = 0 (the other half of
 * a stacked [fake; real] batch).  items: HOST array, count <= MG_LOSS_MAX_ITEMS. */
#define MG_LOSS_MAX_ITEMS 16
typedef struct {
    const float* a;
    const float* b;        /* kind 1 only */
    float* grad;           /* backward only */
    long long n;
    long long zero_tail;   /* backward only */
} mg_loss_item;
size_t mg_loss_multi_workspace(void);
int mg_loss_multi_fwd(int kind, const mg_loss_item* items, int count, float target, float scale, float* loss, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);
int mg_loss_multi_bwd(int kind, const mg_loss_item* items, int count, float target, float scale, const float* grad_out,
                      void* stream);

/* K12  fused Adam over one flat float32 buffer (torch.optim.Adam semantics, no weight decay / amsgrad):
 *      pix2pixHD_model.py:350-351, 363-364; train.py:186-202.  step is 1-based.
 *      grad_scale multiplies g first (1/world_size for DDP, 1/loss_scale for AMP). */
int mg_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                 float eps, int step, float grad_scale, void* stream);

/* hipGraph-replayable variant: the optimiser clock lives in HBM.  state = double[6] {step, lr, lr/(1-beta1^step),
 * sqrt(1-beta2^step), 1-beta1^(step+1), sqrt(1-beta2^(step+1))}; mg_adam_tick advances it on the device (host writes state[1] = lr when the schedule
 * changes), mg_adam_step_dev reads it -- no step-dependent value is baked into a kernel argument. */
int mg_adam_tick(double* state, float beta1, float beta2, void* stream);
/* state[4] = 1 - beta1^(step+1), state[5] = sqrt(1 - beta2^(step+1)) for the clock as it stands (a fresh or restored clock; every
 * tick maintains them afterwards): the terms mg_conv_wgrad_adam_w reads.  The clock is double[6]. */
int mg_adam_prime(double* state, float beta1, float beta2, void* stream);
int mg_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, const double* state, float beta1,
                     float beta2, float eps, float grad_scale, void* stream);

/* torch.cuda.amp.GradScaler on the device (train.py:65-70: one scaler; :183-199: scale(loss).backward(),
 * scaler.step(optimizer) per optimiser, scaler.update() once per iteration) -- no host synchronisation, so the AMP
 * step stays hipGraph-capturable.  scaler: float[2 + MG_SCALER_SLOTS] = {loss scale S, growth tracker,
 * found_inf[slot]...} (one slot per optimiser; the caller initialises {init_scale, 0, 0...}).
 *   mg_scaler_check   found_inf[slot] = 1 if any gradient in g[0..n) is inf / nan  (GradScaler.unscale_'s check)
 *   mg_adam_tick_amp / mg_adam_step_amp   mg_adam_tick / mg_adam_step_dev with the gradients divided by S, and a
 *                     no-op -- parameters, moments and step counter untouched -- when found_inf[slot] != 0
 *   mg_scaler_update  any found_inf: S *= backoff_factor, tracker = 0; else tracker += 1 and, at growth_interval,
 *                     S *= growth_factor, tracker = 0.  Clears every found_inf slot. */
#define MG_SCALER_SLOTS 2
int mg_scaler_check(const float* g, long long n, float* scaler, int slot, void* stream);
int mg_scaler_update(float* scaler, float growth_factor, float backoff_factor, int growth_interval, void* stream);
int mg_adam_tick_amp(double* state, float beta1, float beta2, const float* scaler, int slot, void* stream);
int mg_adam_step_amp(float* p, const float* g, float* m, float* v, long long n, const double* state, float beta1,
                     float beta2, float eps, float grad_scale, const float* scaler, int slot, void* stream);
/* mg_adam_step_amp (scaler != NULL) or mg_adam_step_dev (scaler == NULL) that also writes p16[i] = (float16) p[i] for the
 * updated parameters: the float16 weight operand of the autocast convolutions (train.py --fp16; autocast casts every
 * weight per call, pix2pixHD_model.py:285-301) is refreshed by the optimiser pass that already streams the parameters
 * instead of by one cast launch per layer.  A skipped step (found_inf) leaves p and p16 untouched. */
int mg_adam_step_h(float* p, const float* g, float* m, float* v, void* p16, long long n, const double* state, float beta1,
                   float beta2, float eps, float grad_scale, const float* scaler, int slot, void* stream);

/* Round 6 -- the --fp16 optimiser passes over a SEGMENTED gradient arena (train.py:161-164, 183-199).  Under torch.autocast a
 * convolution's weight / bias gradient is a float16 tensor (the cast's backward widens it into the float32 .grad): its values are
 * float16-rounded and overflow at 65504 -- which is what the reference's GradScaler backs off on.  A segment = a run of the arena
 * [off, off + n) (multiples of 8 elements; device array `segs`) and how its gradient is carried:
 *   MG_GRAD_F32       float32 in g, used as stored (BatchNorm and position-embedding parameters: float32 in the reference too)
 *   MG_GRAD_AUTOCAST  float32 in g, rounded through float16 where it is consumed: finite iff |v| < 65520, Adam reads half(v)
 *   MG_GRAD_F16       float16 in g16 at the same element index, written by mg_conv_wgrad_h16 (half the bytes in both passes)
 * skip_check != 0: the producing kernel already ran the inf / nan test on this segment (mg_conv_wgrad_h16 / mg_conv_wgrad_chk).
 * mg_scaler_check_segs == mg_scaler_check, mg_adam_step_segs == mg_adam_step_h (p16 nullable), one launch each over all
 * segments; n_total (sum of the lengths) sizes the grid. */
#define MG_GRAD_F32 0
#define MG_GRAD_AUTOCAST 1
#define MG_GRAD_F16 2
typedef struct {
    long long off;
    long long n;
    int mode;
    int skip_check;
} mg_grad_seg;
int mg_scaler_check_segs(const float* g, const void* g16, const mg_grad_seg* segs, int nsegs, long long n_total, float* scaler,
                         int slot, void* stream);
int mg_adam_step_segs(float* p, const float* g, const void* g16, float* m, float* v, void* p16, const mg_grad_seg* segs, int nsegs,
                      long long n_total, const double* state, float beta1, float beta2, float eps, float grad_scale,
                      const float* scaler, int slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDCTGAN_HIP_H */
