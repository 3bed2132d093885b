// modelio.hip — the rows of point_cloud.ply (scene/gaussian_model.py:450-493, 541-611) packed from
// and unpacked into the ten stored tensors of a model, one launch each way.
//
// A row is A = 18 + 3 (M - 1) + 7 G float32 columns in save_ply's property order:
//   x y z | nx ny nz (zeros) | f_dc_0..2 | f_rest_* | opacity | scale_0..2 | rot_0..3 |
//   sg_axis_* | sg_sharpness_* | sg_color_* | filter_3D
// Every block is a plain flatten of its tensor's row except f_rest, the reference's
// transpose(1, 2).flatten(1): f_rest_{c (M-1) + k} = features_rest[p, k, c].
//
// Both kernels are gathers through LDS and copy bits (uint32 loads and stores, no arithmetic; the
// one exception is a float64 file column, converted round-to-nearest-even).  A workgroup owns R
// consecutive rows.  Each tensor's values for those rows are one contiguous span of global memory,
// so the tensor side is always coalesced; the row side is the workgroup's R A contiguous words.
//
// pack:   span loads (16 B per lane where the pointers allow) -> ds_write_b32 at [row][column] of a
//         dense R x A tile -> the tile as one run of 16-B stores.  The tile is dense so that the
//         write-out needs no index arithmetic and reads LDS 16 B wide; the price is bank conflicts
//         on the scattered writes of the narrow tensors when A is a multiple of 16 (A = 112: the
//         13 columns of xyz, normals, opacity, scale and filter_3D, 12% of the words).
// unpack: a file row is `stride` bytes, any number, so a block's first byte is in general
//         unaligned.  The block's byte span goes into LDS from the 16-B boundary below it (16-B
//         loads, and single bytes for what is left past the last whole 16 B: nothing outside
//         [rows, rows + P stride) is read), and every value is assembled from the two or three
//         aligned LDS words it lies in (v_alignbyte_b32).  No unaligned global load anywhere.
//
// All global offsets are 64-bit (P A 4 passes 2^31 at 5M Gaussians with SG 7); what is 32-bit is
// an index inside one tile, below 2^15.
#include "gsr_kernels.h"

namespace gsr {

constexpr int kModelThreads = 256;
constexpr int kModelTileBytes = 32 * 1024;  // half the 64-KiB workgroup limit: five workgroups share a CU's LDS
constexpr int kModelMaxRows = 256;

struct ModelField {
    uint32_t* p;     // the tensor [P, w]; pack reads it (NULL: zeros, the normals), unpack writes it
    int w;           // words per Gaussian; 0: absent
    int col;         // its first column in a row
    int tr;          // 0: plain flatten; K: the tensor is [K,3] and the row holds [3,K]
    uint32_t magic;  // floor(2^32 / w) + 1
};
constexpr int kModelFields = 11;
struct ModelLayout {
    ModelField f[kModelFields];
    int A;
};

// (row, column of the file row) of word j of a field's span.  j / w by multiplication: with
// m w = 2^32 + e, 0 < e <= w, umulhi(j, m) = floor(j / w) while j e < 2^32; j and w are below 2^15.
__device__ __forceinline__ void model_place(const ModelField& F, uint32_t j, uint32_t& row, uint32_t& col) {
    row = F.w == 1 ? j : __umulhi(j, F.magic);
    const uint32_t c = j - row * (uint32_t)F.w;
    if (F.tr) {
        const uint32_t k = c / 3u;
        col = (uint32_t)F.col + (c - 3u * k) * (uint32_t)F.tr + k;
    } else {
        col = (uint32_t)F.col + c;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kModelThreads)
    model_pack_rows_kernel(ModelLayout L, long long P, int R, uint32_t* __restrict__ rows) {
    extern __shared__ uint4 s_tile4[];
    uint32_t* s_tile = reinterpret_cast<uint32_t*>(s_tile4);
    const long long r0 = (long long)blockIdx.x * R;
    const uint32_t n = (uint32_t)min((long long)R, P - r0);
    const uint32_t A = (uint32_t)L.A;
#pragma unroll
    for (int f = 0; f < kModelFields; f++) {
        const ModelField F = L.f[f];
        if (F.w == 0) continue;
        const uint32_t span = n * (uint32_t)F.w;
        const uint32_t* src = F.p ? F.p + r0 * F.w : nullptr;
        if (VEC && src) {
            // (R is a multiple of 4 on this path: r0 w words is a multiple of 16 bytes)
            for (uint32_t j = threadIdx.x * 4u; j < span; j += kModelThreads * 4u) {
                uint32_t v[4] = {0u, 0u, 0u, 0u};
                const uint32_t cnt = min(4u, span - j);
                if (cnt == 4u) {
                    const uint4 q = *reinterpret_cast<const uint4*>(src + j);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
                    for (uint32_t e = 0; e < cnt; e++) v[e] = src[j + e];
                }
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) {
                    if (e < cnt) {
                        uint32_t row, col;
                        model_place(F, j + e, row, col);
                        s_tile[row * A + col] = v[e];
                    }
                }
            }
        } else {
            for (uint32_t j = threadIdx.x; j < span; j += kModelThreads) {
                uint32_t row, col;
                model_place(F, j, row, col);
                s_tile[row * A + col] = src ? src[j] : 0u;
            }
        }
    }
    __syncthreads();
    const uint32_t total = n * A;
    uint32_t* dst = rows + r0 * (long long)A;
    if (VEC) {
        const uint32_t whole = total & ~3u;
        for (uint32_t j = threadIdx.x * 4u; j < whole; j += kModelThreads * 4u)
            *reinterpret_cast<uint4*>(dst + j) = s_tile4[j >> 2];
        for (uint32_t j = whole + threadIdx.x; j < total; j += kModelThreads) dst[j] = s_tile[j];
    } else {
        for (uint32_t j = threadIdx.x; j < total; j += kModelThreads) dst[j] = s_tile[j];
    }
}

__global__ void __launch_bounds__(kModelThreads)
    model_unpack_rows_kernel(ModelLayout L, long long P, int R, long long stride, const uint8_t* __restrict__ rows,
                             const int32_t* __restrict__ col_offset, const int32_t* __restrict__ col_type) {
    extern __shared__ uint4 s_tile4[];
    const uint32_t* s_words = reinterpret_cast<const uint32_t*>(s_tile4);
    uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_tile4);
    const long long r0 = (long long)blockIdx.x * R;
    const uint32_t n = (uint32_t)min((long long)R, P - r0);
    // the block's bytes [b0, b1) of `rows` (16-B aligned), staged from a0 = b0 rounded down to 16
    const unsigned long long b0 = (unsigned long long)r0 * (unsigned long long)stride;
    const unsigned long long b1 = b0 + (unsigned long long)n * (unsigned long long)stride;
    const unsigned long long a0 = b0 & ~15ull, whole = b1 & ~15ull;  // (a0 <= whole: a0 is a multiple of 16 below b1)
    const uint32_t lead = (uint32_t)(b0 - a0);
    const uint32_t n16 = (uint32_t)((whole - a0) >> 4), rest = (uint32_t)(b1 - whole);
    const uint4* src16 = reinterpret_cast<const uint4*>(rows + a0);
    for (uint32_t k = threadIdx.x; k < n16; k += kModelThreads) s_tile4[k] = src16[k];
    if (threadIdx.x < rest) s_bytes[(n16 << 4) + threadIdx.x] = rows[whole + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (int f = 0; f < kModelFields; f++) {
        const ModelField F = L.f[f];
        if (F.w == 0 || !F.p) continue;
        const uint32_t span = n * (uint32_t)F.w;
        uint32_t* dst = F.p + r0 * F.w;
        for (uint32_t j = threadIdx.x; j < span; j += kModelThreads) {
            uint32_t row, col;
            model_place(F, j, row, col);
            const int off = col_offset[col];
            uint32_t v = 0u;
            if (off >= 0) {
                const uint32_t a = lead + row * (uint32_t)stride + (uint32_t)off;
                const uint32_t w = a >> 2, sh = a & 3u;
                const uint32_t x0 = s_words[w], x1 = s_words[w + 1];
                v = __builtin_amdgcn_alignbyte(x1, x0, sh);
                if (col_type[col] == 1) {
                    const uint32_t hi = __builtin_amdgcn_alignbyte(s_words[w + 2], x1, sh);
                    v = __float_as_uint((float)__hiloint2double((int)hi, (int)v));  // (round to nearest even)
                }
            }
            dst[j] = v;
        }
    }
}

// ---- host ----

int model_row_floats(int M, int G) {
    if (M < 1 || G < 0 || M > (1 << 20) || G > (1 << 20)) return 0;
    return 18 + 3 * (M - 1) + 7 * G;
}

// Rows per workgroup of the pack kernel for rows of A words: the most that fit the tile, at most
// kModelMaxRows, a multiple of 4 where there are 4 (every span of a block then starts on 16 bytes);
// 0 when not even one row fits.
int model_block_rows(int A) {
    if (A < 1) return 0;
    const int fit = kModelTileBytes / 4 / A, r = fit < kModelMaxRows ? fit : kModelMaxRows;
    return r >= 4 ? r & ~3 : r;
}

// Rows per workgroup of the unpack kernel for file rows of `stride` bytes (the staged span is up
// to 15 bytes of lead, the rows, and the 4 bytes past a last value that its word pair reaches).
int model_unpack_block_rows(long long stride) {
    if (stride < 1 || stride > kModelTileBytes - 32) return 0;
    const long long fit = (kModelTileBytes - 32) / stride;
    return fit < kModelMaxRows ? (int)fit : kModelMaxRows;
}

static ModelLayout model_layout(int M, int G, float* const* t) {
    // t: xyz, features_dc, features_rest, opacity, scaling, rotation, sg_axis, sg_sharpness, sg_color, filter_3D
    const int widths[kModelFields] = {3, 3, 3, 3 * (M - 1), 1, 3, 4, 3 * G, G, 3 * G, 1};
    float* const ptrs[kModelFields] = {t[0], nullptr, t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9]};
    ModelLayout L;
    int col = 0;
    for (int f = 0; f < kModelFields; f++) {
        ModelField& F = L.f[f];
        F.p = reinterpret_cast<uint32_t*>(ptrs[f]);
        F.w = widths[f];
        F.col = col;
        F.tr = f == 3 ? M - 1 : 0;
        F.magic = F.w > 1 ? (uint32_t)(0x100000000ull / (unsigned long long)F.w) + 1u : 0u;
        col += F.w;
    }
    L.A = col;
    return L;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

hipError_t launch_model_pack_rows(long long P, int M, int G, const float* const* tensors, float* rows,
                                  hipStream_t stream) {
    const ModelLayout L = model_layout(M, G, const_cast<float* const*>(tensors));
    const int R = model_block_rows(L.A);
    bool vec = (R & 3) == 0 && aligned16(rows);
    for (int f = 0; f < kModelFields; f++) vec = vec && (L.f[f].w == 0 || aligned16(L.f[f].p));
    const unsigned blocks = (unsigned)((P + R - 1) / R);
    const size_t lds = align_up((size_t)R * L.A * 4, 16);
    if (vec)
        model_pack_rows_kernel<true><<<blocks, kModelThreads, lds, stream>>>(L, P, R, reinterpret_cast<uint32_t*>(rows));
    else
        model_pack_rows_kernel<false><<<blocks, kModelThreads, lds, stream>>>(L, P, R, reinterpret_cast<uint32_t*>(rows));
    return hipGetLastError();
}

hipError_t launch_model_unpack_rows(long long P, int M, int G, long long stride, const uint8_t* rows,
                                    const int32_t* col_offset, const int32_t* col_type, float* const* tensors,
                                    hipStream_t stream) {
    const ModelLayout L = model_layout(M, G, tensors);
    const int R = model_unpack_block_rows(stride);
    const unsigned blocks = (unsigned)((P + R - 1) / R);
    const size_t lds = align_up((size_t)R * stride + 32, 16);
    model_unpack_rows_kernel<<<blocks, kModelThreads, lds, stream>>>(L, P, R, stride, rows, col_offset, col_type);
    return hipGetLastError();
}

}  // namespace gsr
