// WAV payloads to packed float32 rows and back (torchaudio.load(normalize=True) / torchaudio.save, data/audio_dataset.py:37-51, :143,
// generate_audio.py:89-96) for MANY files in shared launches: the payload bytes of every file sit at their own place of one byte
// buffer, the waveforms at aligned starts of one float32 buffer, and a device table of mg_pcm_row says where every row (one channel
// of one file) reads and writes.
//   pcm_decode_rows_kernel   one workgroup = one chunk of MG_MOMENTS_CHUNK frames of one row; thread t owns frames 4t .. 4t+3 (+ 1024 i)
//                            of the chunk, exactly as rows_moments_chunks_kernel (resample_rows.hip) owns samples.  The four raw
//                            samples come from aligned vector loads where the row's bytes allow it (mono S16 / S32 / F32 / F64,
//                            mono U8 / S24 through dwords, stereo S16) and from single bytes otherwise; ONE function (pcm_value) turns raw bits
//                            into the float32, so a row has the same bits through every load path.  MOMENTS: the same pass
//                            accumulates {sum x, sum x^2} in double through block_sum_store<2>; pcm_moments_final_kernel runs
//                            sum_chunks<2> -- bit for bit mg_rows_moments over the decoded window.
//   pcm_encode_rows_kernel   the reverse: one workgroup of 1024 walks one row and writes its channel's bytes of every frame (rows of
//                            one file write disjoint bytes), counting the samples it clamped (or that were NaN) in registers; one
//                            integer sum per row at the end, so the entry point needs no workspace.
// Every window is cut to both of its buffers in WHOLE frames (pcm_cut), a broken row is dead, there are no atomics.
#include <limits.h>
#include <stdint.h>

#include "rows.h"

namespace {

__device__ __forceinline__ int pcm_sample_bytes(long long format) {
    switch (format) {
        case MG_PCM_U8: return 1;
        case MG_PCM_S16: return 2;
        case MG_PCM_S24: return 3;
        case MG_PCM_S32: return 4;
        case MG_PCM_F32: return 4;
        case MG_PCM_F64: return 8;
        default: return 0;
    }
}

// A row cut to its two buffers: `frames` whole frames (0: a dead row), frame f's sample at byte `byte_pos + f * frame_bytes` (the
// channel's offset is inside byte_pos) and at float `sample_pos + f`
struct PcmCut {
    long long byte_pos, sample_pos, frames;
    int frame_bytes, sample_bytes, format;
    bool mono;
};

__device__ __forceinline__ PcmCut pcm_cut(const mg_pcm_row& rw, long long row_byte_pos, long long bytes_total,
                                          long long row_sample_pos, long long samples_total) {
    PcmCut c;
    c.frames = 0;
    c.sample_bytes = pcm_sample_bytes(rw.format);
    c.format = (int)rw.format;
    c.mono = rw.channels == 1;
    c.frame_bytes = 0; c.byte_pos = 0; c.sample_pos = 0;
    if (c.sample_bytes == 0 || rw.channels < 1 || rw.channels > 65535 || rw.channel < 0 || rw.channel >= rw.channels) return c;
    if (rw.frames <= 0 || row_byte_pos < 0 || row_byte_pos >= bytes_total || row_sample_pos < 0 || row_sample_pos >= samples_total)
        return c;
    c.frame_bytes = (int)rw.channels * c.sample_bytes;
    const long long in_bytes = (bytes_total - row_byte_pos) / c.frame_bytes, in_samples = samples_total - row_sample_pos;
    long long n = rw.frames < in_bytes ? rw.frames : in_bytes;
    c.frames = n < in_samples ? n : in_samples;
    c.byte_pos = row_byte_pos + rw.channel * c.sample_bytes;
    c.sample_pos = row_sample_pos;
    return c;
}

// THE conversion: the raw little-endian bits of one sample (lo: its first four bytes, hi: the next four of a float64; bits beyond
// the sample are ignored) -> torchaudio.load's float32.  Integer formats scale by a power of two (exact; S32 rounds to nearest even
// once, in the int -> float conversion), F32 keeps its bits, F64 is one round-to-nearest-even cast.
__device__ __forceinline__ float pcm_value(int format, unsigned lo, unsigned hi) {
    switch (format) {
        case MG_PCM_U8: return (float)((int)(lo & 0xffu) - 128) * 0x1p-7f;
        case MG_PCM_S16: return (float)(short)(lo & 0xffffu) * 0x1p-15f;
        case MG_PCM_S24: return (float)((int)(lo << 8) >> 8) * 0x1p-23f;
        case MG_PCM_S32: return (float)(int)lo * 0x1p-31f;
        case MG_PCM_F32: return __uint_as_float(lo);
        default: return (float)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
}

__device__ __forceinline__ void pcm_load_bytes(const unsigned char* __restrict__ p, int sample_bytes, unsigned& lo, unsigned& hi) {
    lo = 0; hi = 0;
    for (int j = 0; j < sample_bytes && j < 4; ++j) lo |= (unsigned)p[j] << (8 * j);
    for (int j = 4; j < sample_bytes; ++j) hi |= (unsigned)p[j] << (8 * (j - 4));
}

// The raw bits of frames f .. f + 3 of a row (the first n_valid of them exist).  p: the first byte of frame f's sample.
__device__ __forceinline__ void pcm_load_quad(const unsigned char* __restrict__ p, const PcmCut& c, int channel_byte, int n_valid,
                                              unsigned (&lo)[4], unsigned (&hi)[4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = 0; hi[k] = 0; }
    if (n_valid == 4 && c.mono) {
        if ((c.format == MG_PCM_S32 || c.format == MG_PCM_F32) && (a & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            lo[0] = v.x; lo[1] = v.y; lo[2] = v.z; lo[3] = v.w;
            return;
        }
        if (c.format == MG_PCM_S16 && (a & 7) == 0) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            lo[0] = v.x; lo[1] = v.x >> 16; lo[2] = v.y; lo[3] = v.y >> 16;
            return;
        }
        if (c.format == MG_PCM_F64 && (a & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(p), w = *reinterpret_cast<const uint4*>(p + 16);
            lo[0] = v.x; hi[0] = v.y; lo[1] = v.z; hi[1] = v.w; lo[2] = w.x; hi[2] = w.y; lo[3] = w.z; hi[3] = w.w;
            return;
        }
        if (c.format == MG_PCM_S24 && (a & 3) == 0) {                       // 4 frames = 12 bytes = three aligned dwords
            const unsigned* q = reinterpret_cast<const unsigned*>(p);
            const unsigned w0 = q[0], w1 = q[1], w2 = q[2];
            lo[0] = w0; lo[1] = (w0 >> 24) | (w1 << 8); lo[2] = (w1 >> 16) | (w2 << 16); lo[3] = w2 >> 8;
            return;
        }
        if (c.format == MG_PCM_U8 && (a & 3) == 0) {
            const unsigned w = *reinterpret_cast<const unsigned*>(p);
            lo[0] = w; lo[1] = w >> 8; lo[2] = w >> 16; lo[3] = w >> 24;
            return;
        }
    }
    if (n_valid == 4 && c.format == MG_PCM_S16 && c.frame_bytes == 4 && ((a - channel_byte) & 15) == 0) {   // stereo: a frame is a dword
        const uint4 v = *reinterpret_cast<const uint4*>(p - channel_byte);
        const int sh = 8 * channel_byte;
        lo[0] = v.x >> sh; lo[1] = v.y >> sh; lo[2] = v.z >> sh; lo[3] = v.w >> sh;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n_valid) pcm_load_bytes(p + (long long)k * c.frame_bytes, c.sample_bytes, lo[k], hi[k]);
}

template <bool MOMENTS>
__global__ __launch_bounds__(256) void pcm_decode_rows_kernel(const unsigned char* __restrict__ bytes, long long bytes_total,
                                                              const mg_pcm_row* __restrict__ rows, int n_rows, int max_chunks,
                                                              float* __restrict__ out, long long out_total, bool out_al16,
                                                              double* __restrict__ partial) {
    __shared__ double red[4][2];
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_pcm_row rw = rows[r];
        const PcmCut cut = pcm_cut(rw, rw.src_pos, bytes_total, rw.dst_pos, out_total);
        if (cut.frames <= 0) continue;
        const int channel_byte = (int)(rw.channel * cut.sample_bytes);
        const int n_chunks = row_chunks(cut.frames, max_chunks);
        for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            const long long base = (long long)c * kChunk;                  // first frame of the chunk
            const int n = (int)(cut.frames - base < kChunk ? cut.frames - base : kChunk);
            double acc[2] = {0.0, 0.0};                                     // sum x, sum x^2
            for (int i = 4 * threadIdx.x; i < n; i += 4 * 256) {
                const int n_valid = n - i < 4 ? n - i : 4;
                unsigned lo[4], hi[4];
                pcm_load_quad(bytes + cut.byte_pos + (base + i) * cut.frame_bytes, cut, channel_byte, n_valid, lo, hi);
                float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k < n_valid) e[k] = pcm_value(cut.format, lo[k], hi[k]);
                float* o = out + cut.sample_pos + base + i;
                if (out_al16 && n_valid == 4 && ((cut.sample_pos + base + i) & 3) == 0) {
                    *reinterpret_cast<float4*>(o) = make_float4(e[0], e[1], e[2], e[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k < n_valid) o[k] = e[k];
                }
                if (MOMENTS) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double d = (double)e[k]; acc[0] += d; acc[1] += d * d; }   // (missing: adds 0)
                }
            }
            if (MOMENTS) block_sum_store<2>(acc, red, partial + ((size_t)r * max_chunks + c) * 2);
        }
    }
}

__global__ __launch_bounds__(256) void pcm_moments_final_kernel(const mg_pcm_row* __restrict__ rows, long long bytes_total,
                                                                long long out_total, int n_rows, int max_chunks,
                                                                const double* __restrict__ partial, double* __restrict__ moments) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const mg_pcm_row rw = rows[r];
    const PcmCut cut = pcm_cut(rw, rw.src_pos, bytes_total, rw.dst_pos, out_total);
    sum_chunks<2>(partial + (size_t)r * max_chunks * 2, row_chunks(cut.frames, max_chunks), moments + 2 * (size_t)r);
}

// clamp(rint(x 2^(bits - 1)), -2^(bits - 1), 2^(bits - 1) - 1): the product is exact (a power of two), rintf rounds half to even,
// NaN becomes 0; `clipped` counts the clamped and the NaN samples
__device__ __forceinline__ int pcm_quantise(float x, float scale, int& clipped) {
    if (x != x) { ++clipped; return 0; }
    float y = rintf(x * scale);
    if (y > scale - 1.0f) { y = scale - 1.0f; ++clipped; }
    else if (y < -scale) { y = -scale; ++clipped; }
    return (int)y;
}

constexpr int kEncodeThreads = 1024;       // one workgroup walks a row: sixteen waves keep a CU busy where a pack has few rows per CU

__global__ __launch_bounds__(kEncodeThreads) void pcm_encode_rows_kernel(const float* __restrict__ x, long long x_total,
                                                              const mg_pcm_row* __restrict__ rows, int n_rows,
                                                              unsigned char* __restrict__ bytes, long long bytes_total,
                                                              long long* __restrict__ clipped) {
    __shared__ long long red[kEncodeThreads / 64];
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const mg_pcm_row rw = rows[r];
        PcmCut cut = pcm_cut(rw, rw.dst_pos, bytes_total, rw.src_pos, x_total);
        if (cut.format != MG_PCM_F32 && cut.format != MG_PCM_S16 && cut.format != MG_PCM_S24) cut.frames = 0;   // (a dead row)
        const float scale = cut.format == MG_PCM_S16 ? 32768.0f : 8388608.0f;
        int count = 0;
        for (long long f = 4 * (long long)threadIdx.x; f < cut.frames; f += 4 * kEncodeThreads) {
            const int n_valid = (int)(cut.frames - f < 4 ? cut.frames - f : 4);
            const float* src = x + cut.sample_pos + f;
            unsigned char* p = bytes + cut.byte_pos + f * cut.frame_bytes;
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n_valid)
                    v[k] = cut.format == MG_PCM_F32 ? __float_as_uint(src[k]) : (unsigned)pcm_quantise(src[k], scale, count);
            if (n_valid == 4 && cut.mono && cut.format == MG_PCM_F32 && (a & 15) == 0) {
                *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
            } else if (n_valid == 4 && cut.mono && cut.format == MG_PCM_S16 && (a & 7) == 0) {
                *reinterpret_cast<uint2*>(p) = make_uint2((v[0] & 0xffffu) | (v[1] << 16), (v[2] & 0xffffu) | (v[3] << 16));
            } else if (n_valid == 4 && cut.mono && cut.format == MG_PCM_S24 && (a & 3) == 0) {
                unsigned* q = reinterpret_cast<unsigned*>(p);
                q[0] = (v[0] & 0xffffffu) | (v[1] << 24);
                q[1] = ((v[1] >> 8) & 0xffffu) | (v[2] << 16);
                q[2] = ((v[2] >> 16) & 0xffu) | (v[3] << 8);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n_valid)
                        for (int j = 0; j < cut.sample_bytes; ++j) p[(long long)k * cut.frame_bytes + j] = (unsigned char)(v[k] >> (8 * j));
            }
        }
        // the row's count: every wave, then the waves in ascending order (integers: any order gives the same sum)
        long long s = count;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long total = 0;
            for (int w = 0; w < kEncodeThreads / 64; ++w) total += red[w];
            clipped[r] = total;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_pcm_decode_rows_workspace(int n_rows, long long max_frames) {
    if (n_rows <= 0 || max_frames <= 0) return 0;
    return (size_t)n_rows * (size_t)((max_frames + kChunk - 1) / kChunk) * 2 * sizeof(double);
}

int mg_pcm_decode_rows(const void* bytes, long long bytes_total, const mg_pcm_row* rows, int n_rows, long long max_frames,
                       float* out, long long out_total, double* moments, void* workspace, size_t workspace_bytes, void* stream) {
    if (!bytes || !rows || !out || n_rows <= 0 || bytes_total <= 0 || out_total <= 0 || max_frames <= 0) return MG_ERR_ARG;
    const long long max_chunks = (max_frames + kChunk - 1) / kChunk;
    if (max_chunks > INT_MAX) return MG_ERR_ARG;
    if (moments && (!workspace || workspace_bytes < mg_pcm_decode_rows_workspace(n_rows, max_frames))) return MG_ERR_ARG;
    if (moments && (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return MG_ERR_ARG;
    const unsigned char* b = static_cast<const unsigned char*>(bytes);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid = rows_grid(n_rows, max_frames, kChunk);
    hipStream_t st = (hipStream_t)stream;
    if (moments) {
        hipLaunchKernelGGL(pcm_decode_rows_kernel<true>, grid, dim3(256), 0, st, b, bytes_total, rows, n_rows, (int)max_chunks, out,
                           out_total, al16(out), partial);
        MG_CHECK_LAUNCH();
        hipLaunchKernelGGL(pcm_moments_final_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, rows, bytes_total,
                           out_total, n_rows, (int)max_chunks, partial, moments);
    } else {
        hipLaunchKernelGGL(pcm_decode_rows_kernel<false>, grid, dim3(256), 0, st, b, bytes_total, rows, n_rows, (int)max_chunks, out,
                           out_total, al16(out), partial);
    }
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_pcm_encode_rows(const float* x, long long x_total, const mg_pcm_row* rows, int n_rows, long long max_frames, void* bytes,
                       long long bytes_total, long long* clipped, void* stream) {
    if (!x || !rows || !bytes || !clipped || n_rows <= 0 || x_total <= 0 || bytes_total <= 0 || max_frames <= 0) return MG_ERR_ARG;
    const unsigned blocks = (unsigned)(n_rows < 65535 ? n_rows : 65535);
    hipLaunchKernelGGL(pcm_encode_rows_kernel, dim3(blocks), dim3(kEncodeThreads), 0, (hipStream_t)stream, x, x_total, rows, n_rows,
                       static_cast<unsigned char*>(bytes), bytes_total, clipped);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
