// scd_input_grad: data grad of the channel-padded first layer, dL/dx of conv0 written straight into the callers'
// NCHW fp32 tensors.
//
//   gx[n][j][y][x] = sum_{o < C0} sum_{ky, kx < 3} dy[n][y+1-ky][x+1-kx][o] * w[o][wc+j][ky][kx]     (zero padding)
//
// The GEMM behind it is M = pixels, N = cin <= 16 real bands, K = 9 * C0: far narrower than the 64-channel blocks of
// the halo conv tiles.  One workgroup owns a TH x TW tile of output pixels, one pixel per thread.  Per 32-channel
// chunk of dy it stages the (TH+2) x (TW+2) halo in LDS once (fp32; a bf16 element widens exactly) and every tap
// reads it from there, so a dy element leaves HBM once per launch apart from the tile's halo ring; the next chunk's
// loads are in flight while the current one is multiplied.  The weights are
// read as the module holds them (OIHW fp32, < 40 KB): their index is uniform over the workgroup, so they travel
// through the scalar cache and enter each fma as a scalar operand -- no pack pass, no pack-cache entry, no LDS.  The
// arithmetic is one fp32 fma chain per output (k order: channel, ky, kx), for either storage type: nothing is
// rounded to bf16.  The kernel is instantiated per exact cin, so no lane multiplies by a padded zero channel.
// Plain fma, not a 16-wide MFMA column: measured 3.3x faster than the generic igemm launch at 5 bands, and bound by
// the fma rate, 1.95x off the byte bound (DESIGN.md section 3.3b has the numbers and what an MFMA column would buy).
#include "common.h"

namespace scd {
namespace {

constexpr int IG_TW = 32;                 // tile width: one 128-byte store row per output channel
constexpr int IG_TH = 8;                  // tile height
constexpr int IG_PY = 1;                  // vertically adjacent output pixels per thread.  2 shares halo rows and
                                          // weights between them but needs 255 registers: measured 2.5x slower
constexpr int IG_THREADS = IG_TW * IG_TH / IG_PY;
constexpr int IG_KC = 32;                 // dy channels per staged chunk: one 128-byte line per fp32 pixel
constexpr int IG_PITCH = IG_KC + 4;       // floats per staged pixel: 16-byte rows; 36 i mod 64 hits every 4-bank group
                                          // once per 16 lanes, so the ds_read_b128 of a row of pixels is conflict-free
constexpr int IG_JG = 4;                  // bands per weight step: 36 scalar registers
constexpr int IG_HW = IG_TW + 2, IG_HH = IG_TH + 2;
constexpr int IG_QUADS = IG_HH * IG_HW * (IG_KC / 4);            // channel quads of one staged chunk
constexpr int IG_STAGE = (IG_QUADS + IG_THREADS - 1) / IG_THREADS;  // ... per thread
constexpr int IG_LDS_BYTES = IG_HH * IG_HW * IG_PITCH * 4;
static_assert(IG_LDS_BYTES <= 160 * 1024 / 3, "input_grad: three workgroups per CU must fit the 160 KiB LDS");
static_assert(IG_TH % IG_PY == 0 && IG_THREADS % 64 == 0, "input_grad: whole waves, whole row groups");
static_assert(IG_PITCH % 4 == 0, "input_grad: staged pixels must stay 16-byte aligned");

struct IGDst {
    float *dst;
    int dst_c, c_begin, c_count, w_c, n_begin, n_count;
};

struct IGParams {
    const void *dy;
    int n, h, w, c0, ldc;
    const float *wt;  // OIHW [c0][cin][3][3]
    int tiles_x;
    IGDst dst[2];
};

template <class T, int CIN>
__global__ __launch_bounds__(IG_THREADS) void input_grad_kernel(const IGParams p) {
    __shared__ __attribute__((aligned(16))) float halo[IG_HH * IG_HW * IG_PITCH];
    const int tid = threadIdx.x;
    const int lx = tid & (IG_TW - 1), ly = (tid / IG_TW) * IG_PY;  // the thread's first output row
    const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int y0 = tile_y * IG_TH, x0 = tile_x * IG_TW;
    const int img = blockIdx.y;
    // 64-bit element offsets throughout: a view of 2 GiB and more is addressed like any other
    const T *const dy = static_cast<const T *>(p.dy) + size_t(img) * p.h * p.w * p.ldc;
    const float *__restrict__ const wt = p.wt;

    float acc[IG_PY][CIN];
#pragma unroll
    for (int k = 0; k < IG_PY; ++k)
#pragma unroll
        for (int j = 0; j < CIN; ++j) acc[k][j] = 0.f;

    // The halo of channels [cb, cb + 32) as 8 quads per pixel; quads past C0 and pixels past the border are zero.
    bnf4 v[IG_STAGE];
    const auto fetch = [&](int cb) {  // every load is issued before anything waits for one
#pragma unroll
        for (int i = 0; i < IG_STAGE; ++i) {
            const int q = tid + i * IG_THREADS;
            const int c4 = (q & (IG_KC / 4 - 1)) * 4, px = q / (IG_KC / 4);
            const int r = px / IG_HW, c = px - r * IG_HW;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            v[i] = bnf4{0.f, 0.f, 0.f, 0.f};
            if (q < IG_QUADS && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w && cb + c4 < p.c0)
                v[i] = ld4(dy + (size_t(gy) * p.w + gx) * p.ldc + cb + c4);
        }
    };
    const auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < IG_STAGE; ++i) {
            const int q = tid + i * IG_THREADS;
            if (q < IG_QUADS)
                *reinterpret_cast<bnf4 *>(&halo[(q / (IG_KC / 4)) * IG_PITCH + (q & (IG_KC / 4 - 1)) * 4]) = v[i];
        }
    };
    fetch(0);
    for (int cb = 0; cb < p.c0; cb += IG_KC) {
        if (cb) __syncthreads();  // every tap of the previous chunk has been read
        stage();
        __syncthreads();
        if (cb + IG_KC < p.c0) fetch(cb + IG_KC);  // the next chunk travels while this one is multiplied
        const int nq = min(IG_KC, p.c0 - cb) / 4;
        for (int q4 = 0; q4 < nq; ++q4) {
            // output (y, x) reads dy(y + 1 - ky, x + 1 - kx): halo row (ly + k) + 2 - ky, column lx + 2 - kx
            bnf4 d[IG_PY + 2][3];
#pragma unroll
            for (int m = 0; m < IG_PY + 2; ++m)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    d[m][c] = *reinterpret_cast<const bnf4 *>(&halo[((ly + m) * IG_HW + lx + c) * IG_PITCH + q4 * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *const wo = wt + size_t(cb + q4 * 4 + e) * (CIN * 9);
                // the weights of IG_JG bands (9 * IG_JG consecutive floats) per step: what the scalar file holds
#pragma unroll
                for (int j0 = 0; j0 < CIN; j0 += IG_JG) {
#pragma unroll
                    for (int j = j0; j < (j0 + IG_JG < CIN ? j0 + IG_JG : CIN); ++j) {
#pragma unroll
                        for (int t = 0; t < 9; ++t) {
#pragma unroll
                            for (int k = 0; k < IG_PY; ++k)
                                acc[k][j] = fmaf(d[k + 2 - t / 3][2 - t % 3][e], wo[j * 9 + t], acc[k][j]);
                        }
                    }
                }
            }
        }
    }

    const int x = x0 + lx;
    if (x >= p.w) return;
    const size_t plane = size_t(p.h) * p.w;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const IGDst &d = p.dst[r];
        if (d.dst == nullptr || img < d.n_begin || img >= d.n_begin + d.n_count) continue;
        float *const base = d.dst + (size_t(img - d.n_begin) * d.dst_c + d.c_begin) * plane + x;
#pragma unroll
        for (int k = 0; k < IG_PY; ++k) {
            const int y = y0 + ly + k;
            if (y >= p.h) break;
#pragma unroll
            for (int j = 0; j < CIN; ++j) {
                if (j >= d.w_c && j < d.w_c + d.c_count) base[size_t(j - d.w_c) * plane + size_t(y) * p.w] = acc[k][j];
            }
        }
    }
}

template <class T, int CIN>
void launch_cin(const IGParams &p, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((input_grad_kernel<T, CIN>), grid, dim3(IG_THREADS), 0, s, p);
}

template <class T>
void launch(const IGParams &p, int cin, dim3 grid, hipStream_t s) {
    switch (cin) {
#define SCD_IG_CASE(k) \
    case k:            \
        return launch_cin<T, k>(p, grid, s);
        SCD_IG_CASE(1) SCD_IG_CASE(2) SCD_IG_CASE(3) SCD_IG_CASE(4) SCD_IG_CASE(5) SCD_IG_CASE(6) SCD_IG_CASE(7)
        SCD_IG_CASE(8) SCD_IG_CASE(9) SCD_IG_CASE(10) SCD_IG_CASE(11) SCD_IG_CASE(12) SCD_IG_CASE(13)
        SCD_IG_CASE(14) SCD_IG_CASE(15) SCD_IG_CASE(16)
#undef SCD_IG_CASE
    }
}

// Every host-side check of a descriptor; no device call, no pointer dereferenced.
int validate(const scd_input_grad_t *d) {
    if (d == nullptr) {
        set_error("input_grad: null descriptor");
        return SCD_ERR_ARG;
    }
    SCD_TRY(check_view(d->dy, "input_grad: dy"));
    if (d->dy.c < 8 || (d->dy.c & 7)) {
        set_error("input_grad: dy.c = %d must be a multiple of 8 (the first layer's width)", d->dy.c);
        return SCD_ERR_ARG;
    }
    if (d->cin < 1 || d->cin > 16) {
        set_error("input_grad: cin = %d must be in [1, 16]", d->cin);
        return SCD_ERR_ARG;
    }
    if (d->w == nullptr || (reinterpret_cast<uintptr_t>(d->w) & 3u)) {
        set_error("input_grad: w must be a 4-byte aligned OIHW fp32 weight");
        return SCD_ERR_ARG;
    }
    if (d->dy.n > 65535 || int64_t(d->dy.h) * d->dy.w > (int64_t(1) << 30)) {
        set_error("input_grad: n must be <= 65535 and h*w <= 2^30");
        return SCD_ERR_ARG;
    }
    int live = 0;
    for (int r = 0; r < 2; ++r) {
        const scd_input_grad_dst_t &t = d->dst[r];
        if (t.dst == nullptr) continue;
        ++live;
        if (reinterpret_cast<uintptr_t>(t.dst) & 3u) {
            set_error("input_grad: dst[%d] must be 4-byte aligned", r);
            return SCD_ERR_ALIGN;
        }
        if (t.dst_c < 1 || t.c_begin < 0 || t.c_count < 1 || int64_t(t.c_begin) + t.c_count > t.dst_c) {
            set_error("input_grad: dst[%d] channels [%d, %d + %d) do not fit dst_c = %d", r, t.c_begin, t.c_begin,
                      t.c_count, t.dst_c);
            return SCD_ERR_ARG;
        }
        if (t.w_c < 0 || int64_t(t.w_c) + t.c_count > d->cin) {
            set_error("input_grad: dst[%d] weight channels [%d, %d + %d) do not fit cin = %d", r, t.w_c, t.w_c,
                      t.c_count, d->cin);
            return SCD_ERR_ARG;
        }
        if (t.n_begin < 0 || t.n_count < 1 || int64_t(t.n_begin) + t.n_count > d->dy.n) {
            set_error("input_grad: dst[%d] images [%d, %d + %d) do not fit dy.n = %d", r, t.n_begin, t.n_begin,
                      t.n_count, d->dy.n);
            return SCD_ERR_ARG;
        }
    }
    if (live == 0) {
        set_error("input_grad: both destination records are null");
        return SCD_ERR_ARG;
    }
    return SCD_OK;
}

}  // namespace
}  // namespace scd

extern "C" int scd_input_grad_supported(const scd_input_grad_t *d) {
    using namespace scd;
    const int rc = validate(d);
    if (rc == SCD_OK) clear_error();
    return rc == SCD_OK ? 1 : 0;
}

extern "C" int scd_input_grad(const scd_input_grad_t *d, scd_stream_t stream) {
    using namespace scd;
    SCD_TRY(validate(d));
    IGParams p;
    p.dy = d->dy.data;
    p.n = d->dy.n, p.h = d->dy.h, p.w = d->dy.w, p.c0 = d->dy.c, p.ldc = d->dy.ldc;
    p.wt = d->w;
    p.tiles_x = (p.w + IG_TW - 1) / IG_TW;
    for (int r = 0; r < 2; ++r) {
        const scd_input_grad_dst_t &t = d->dst[r];
        p.dst[r] = IGDst{t.dst, t.dst_c, t.c_begin, t.c_count, t.w_c, t.n_begin, t.n_count};
    }
    const int64_t tiles = int64_t(p.tiles_x) * ((p.h + IG_TH - 1) / IG_TH);  // < 2^31 by the h*w check
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(p.n));
    SCD_WITH_T(d->dy.dtype, T, launch<T>(p, d->cin, grid, as_stream(stream)));
    return launch_status("input_grad");
}
