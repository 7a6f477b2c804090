// The loss family: the criteria utils/loss_functions.py:6-33 registers beside power_jaccard_loss (soft dice 36-56,
// dice-like 129-138, IoU 153-162, balanced soft dice 184-198, nn.BCEWithLogitsLoss, nn.MSELoss) and the MMCR `L2`
// consistency branch (train_semisupervised.py:101-102), as one fused multi-term forward / from-sums / backward trio
// with the term semantics of jaccard_multi_* (loss_f32.hip): per-term sample subsets selected on the device, soft
// targets that receive a gradient, and the exact-DataParallel "sum the rows over the ranks, re-form the loss" path.
//
// p = sigmoid(logit), t = target (or sigmoid(target logit)), sums over the selected elements, N = their number:
//   ratio kinds      loss from {I = sum p t, P = sum p, T = sum t, Q = sum p^2 + t^2}; dL/dp_i = a + b t_i + c p_i with
//                    a, b, c functions of the sums only (lf_form_row), dL/dt_i the same with p and t swapped
//   pointwise kinds  loss = E / N, E = sum of the per-element expression
// Every reduction is a fixed-order tree (wave shuffle, LDS, one record per block, double finalize): no atomics.
#include "common.h"

namespace scd {

constexpr int LF_MAX = 4;        // terms per call
constexpr int LF_BLOCKS = 1024;  // partial-record blocks per term, at most (fewer: one 16-byte vector per thread)
constexpr int LF_REC = 4;        // floats per partial record
constexpr int LF_ROW = 8;        // floats per sums row: {I | E, P, T, Q, selected samples, a, b, c}

// which sums a kind accumulates
enum { LF_CLS_IQ = 0, LF_CLS_PTI = 1, LF_CLS_BCE = 2, LF_CLS_MSE = 3 };

struct LTerms {
    scd_loss_term_t t[LF_MAX];
    int n;
};

typedef float lf4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int lf_class(int kind) {
    switch (kind) {
        case SCD_LOSS_POWER_JACCARD:
        case SCD_LOSS_DICE_LIKE: return LF_CLS_IQ;
        case SCD_LOSS_BCE_LOGITS: return LF_CLS_BCE;
        case SCD_LOSS_MSE: return LF_CLS_MSE;
        default: return LF_CLS_PTI;
    }
}

__device__ __forceinline__ float lf_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ bool lf_selected(int select, const uint8_t *labeled, int s) {
    return select == 0 || ((labeled[s] != 0) == (select == 1));
}

// sample of flat element i; `small`: the whole tensor has < 2^31 elements (32-bit division)
__device__ __forceinline__ int lf_sample(int64_t i, int64_t pixels, bool small) {
    return small ? int(uint32_t(i) / uint32_t(pixels)) : int(i / pixels);
}

// 0: no element of the vector at i is selected, 1: all four are, 2: the vector crosses a sample boundary
__device__ __forceinline__ int lf_vec_state(int select, const uint8_t *labeled, int64_t i, int64_t pixels,
                                            bool small) {
    if (select == 0) return 1;
    const int s = lf_sample(i, pixels, small);
    if (i - int64_t(s) * pixels + 3 >= pixels) return 2;
    return lf_selected(select, labeled, s) ? 1 : 0;
}

constexpr uint32_t LF_ALL_VALID = 0x01010101u;  // the mask word of a term without a mask

// byte j of a little-endian mask word: any non-zero byte means the element counts
__device__ __forceinline__ bool lf_valid_byte(uint32_t m, int j) { return ((m >> (8 * j)) & 0xffu) != 0u; }

template <int CLS>
__device__ __forceinline__ void lf_acc(const scd_loss_term_t &T, float x, float tv, float &a0, float &a1, float &a2) {
    const float t = T.soft_target ? lf_sigmoid(tv) : tv;
    if (CLS == LF_CLS_IQ) {
        const float p = lf_sigmoid(x);
        a0 = fmaf(p, t, a0);
        a1 += p * p + t * t;
    } else if (CLS == LF_CLS_PTI) {
        const float p = lf_sigmoid(x);
        a0 = fmaf(p, t, a0);
        a1 += p;
        a2 += t;
    } else if (CLS == LF_CLS_BCE) {  // the stable form: finite for logits of +-100
        a0 += fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    } else {
        const float d = (T.sigmoid_input ? lf_sigmoid(x) : x) - t;
        a0 = fmaf(d, d, a0);
    }
}

// MASKED: `valid` (one byte per element, non-zero = the element counts; NULL = every element) joins the sample
// selection, and cnt receives the number of elements accumulated.  An invalid element is skipped by a branch, never
// multiplied by 0: whatever its logit / target hold (NaN, Inf) stays out of the arithmetic.  The elements that are
// accumulated take the unmasked sweep's order, so an all-ones mask gives the unmasked sums bit for bit.  With `vec`
// the mask pointer is 4-byte aligned (lf_load_masked): one 4-byte mask word per 16-byte vector.
template <int CLS, bool MASKED>
__device__ __forceinline__ void lf_partial_sweep(const scd_loss_term_t &T, const uint8_t *__restrict__ labeled,
                                                 const uint8_t *__restrict__ valid, int64_t n, int64_t pixels,
                                                 bool vec, float &a0, float &a1, float &a2, uint32_t &cnt) {
    const bool small = n < (int64_t(1) << 31);
    const int64_t tid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t nvec = vec ? n >> 2 : 0;
    int64_t v = tid;
    // every sample: no per-vector decisions, two vectors in flight (same summation order)
    if (!MASKED && T.select == 0) {
        for (; v + stride < nvec; v += 2 * stride) {
            const lf4 x0 = *reinterpret_cast<const lf4 *>(T.logits + (v << 2));
            const lf4 t0 = *reinterpret_cast<const lf4 *>(T.target + (v << 2));
            const lf4 x1 = *reinterpret_cast<const lf4 *>(T.logits + ((v + stride) << 2));
            const lf4 t1 = *reinterpret_cast<const lf4 *>(T.target + ((v + stride) << 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) lf_acc<CLS>(T, x0[j], t0[j], a0, a1, a2);
#pragma unroll
            for (int j = 0; j < 4; ++j) lf_acc<CLS>(T, x1[j], t1[j], a0, a1, a2);
        }
    }
    for (; v < nvec; v += stride) {
        const int64_t i = v << 2;
        const int st = lf_vec_state(T.select, labeled, i, pixels, small);
        if (st == 0) continue;
        uint32_t m = LF_ALL_VALID;
        if (MASKED) {
            if (valid) m = *reinterpret_cast<const uint32_t *>(valid + i);
            if (m == 0u) continue;  // nothing of this vector counts: neither float load is issued
        }
        const lf4 x = *reinterpret_cast<const lf4 *>(T.logits + i);
        const lf4 tv = *reinterpret_cast<const lf4 *>(T.target + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (st == 2 && !lf_selected(T.select, labeled, lf_sample(i + j, pixels, small))) continue;
            if (MASKED) {
                if (!lf_valid_byte(m, j)) continue;
                ++cnt;
            }
            lf_acc<CLS>(T, x[j], tv[j], a0, a1, a2);
        }
    }
    for (int64_t i = (nvec << 2) + tid; i < n; i += stride) {  // tail, or everything without 16-byte alignment
        if (T.select != 0 && !lf_selected(T.select, labeled, lf_sample(i, pixels, small))) continue;
        if (MASKED) {
            if (valid && valid[i] == 0) continue;
            ++cnt;
        }
        lf_acc<CLS>(T, T.logits[i], T.target[i], a0, a1, a2);
    }
}

__device__ __forceinline__ float lf_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

struct LMasks {
    const uint8_t *v[LF_MAX];
};

// rec[term][block] = this block's {I | E, P | Q, T, 0} over its selected elements; MASKED: over its selected valid
// elements, and crec[term][block] = their number (an integer: exact at any size)
template <bool MASKED>
__device__ __forceinline__ void lf_partial_body(const LTerms &terms, const uint8_t *__restrict__ labeled,
                                                const uint8_t *__restrict__ valid, int n_samples, int64_t pixels,
                                                unsigned vec_mask, float *__restrict__ rec,
                                                unsigned long long *__restrict__ crec) {
    const scd_loss_term_t T = terms.t[blockIdx.y];
    const int64_t n = int64_t(n_samples) * pixels;
    const bool vec = (vec_mask >> blockIdx.y) & 1u;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    uint32_t cnt = 0;
#define SCD_LF_SWEEP(CLS) lf_partial_sweep<CLS, MASKED>(T, labeled, valid, n, pixels, vec, a0, a1, a2, cnt)
    switch (lf_class(T.kind)) {
        case LF_CLS_IQ: SCD_LF_SWEEP(LF_CLS_IQ); break;
        case LF_CLS_PTI: SCD_LF_SWEEP(LF_CLS_PTI); break;
        case LF_CLS_BCE: SCD_LF_SWEEP(LF_CLS_BCE); break;
        default: SCD_LF_SWEEP(LF_CLS_MSE); break;
    }
#undef SCD_LF_SWEEP
    __shared__ float sw[4][3];
    __shared__ unsigned long long sc[4];
    a0 = lf_wave_sum(a0);
    a1 = lf_wave_sum(a1);
    a2 = lf_wave_sum(a2);
    unsigned long long c = cnt;
    if (MASKED) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sw[threadIdx.x >> 6][0] = a0;
        sw[threadIdx.x >> 6][1] = a1;
        sw[threadIdx.x >> 6][2] = a2;
        if (MASKED) sc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lf4 r;
        r[0] = (sw[0][0] + sw[1][0]) + (sw[2][0] + sw[3][0]);
        r[1] = (sw[0][1] + sw[1][1]) + (sw[2][1] + sw[3][1]);
        r[2] = (sw[0][2] + sw[1][2]) + (sw[2][2] + sw[3][2]);
        r[3] = 0.f;
        *reinterpret_cast<lf4 *>(rec + (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * LF_REC) = r;
        if (MASKED) crec[size_t(blockIdx.y) * gridDim.x + blockIdx.x] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    }
}

__global__ __launch_bounds__(256) void loss_multi_partial(LTerms terms, const uint8_t *__restrict__ labeled,
                                                          int n_samples, int64_t pixels, unsigned vec_mask,
                                                          float *__restrict__ rec) {
    lf_partial_body<false>(terms, labeled, nullptr, n_samples, pixels, vec_mask, rec, nullptr);
}

__global__ __launch_bounds__(256) void loss_masked_partial(LTerms terms, LMasks masks,
                                                           const uint8_t *__restrict__ labeled, int n_samples,
                                                           int64_t pixels, unsigned vec_mask, float *__restrict__ rec,
                                                           unsigned long long *__restrict__ crec) {
    lf_partial_body<true>(terms, labeled, masks.v[blockIdx.y], n_samples, pixels, vec_mask, rec, crec);
}

// The sums {I | E, P, T, Q, selected samples} of one row -> its loss, and the backward's coefficients into row[5..7].
// In double from the float sums, so a row formed on one device and a row summed over ranks take the same arithmetic.
// N = samples * pixels is formed here: a sample count survives an fp32 all-reduce exactly, an element count of
// 8 ranks x 64 x 256^2 would not.
// The masked calls pass N, the number of selected valid elements, from their integer count (lf_form_row_n).
__device__ double lf_form_row_n(int kind, float *row, double N, float fI, float fP, float fT, float fQ) {
    const double I = fI, P = fP, T = fT, Q = fQ, e = 1e-6;
    double L = 0, a = 0, b = 0, c = 0;
    if (N > 0) {  // one double division per denominator (this runs on a single lane): r = 1 / denominator
        switch (kind) {
            case SCD_LOSS_POWER_JACCARD: {  // D = Q - I + e
                const double r = 1 / (Q - I + e);
                L = 1 - I * r;
                b = -r - I * r * r;
                c = 2 * I * r * r;
            } break;
            case SCD_LOSS_DICE_LIKE: {  // W = Q + e
                const double r = 1 / (Q + e);
                L = 1 - 2 * I * r;
                b = -2 * r;
                c = 4 * I * r * r;
            } break;
            case SCD_LOSS_SOFT_DICE: {  // U = P + T + e
                const double r = 1 / (P + T + e);
                L = 1 - (2 * I + e) * r;
                a = (2 * I + e) * r * r;
                b = -2 * r;
            } break;
            case SCD_LOSS_IOU: {  // V = P + T - I + e
                const double r = 1 / (P + T - I + e);
                L = 1 - I * r;
                a = I * r * r;
                b = -r - I * r * r;
            } break;
            case SCD_LOSS_SOFT_DICE_BALANCED: {  // U = P + T + e, Un = 2N - P - T + e, Nn = N - P - T + I
                const double r = 1 / (P + T + e), rn = 1 / (2 * N - P - T + e), Nn = N - P - T + I;
                L = 1 - 2 * I * r - 2 * Nn * rn;
                a = 2 * I * r * r + 2 * rn - 2 * Nn * rn * rn;
                b = -2 * r - 2 * rn;
            } break;
            default: {  // pointwise: mean over the selected elements
                const double r = 1 / N;
                L = I * r;
                a = r;
            } break;
        }
    }
    row[5] = float(a);
    row[6] = float(b);
    row[7] = float(c);
    return L;
}

__device__ double lf_form_row(int kind, float *row, int64_t pixels, float fI, float fP, float fT, float fQ,
                              float count) {
    return lf_form_row_n(kind, row, double(count) * double(pixels), fI, fP, fT, fQ);
}

// MASKED: counts[k] = the sum of the term's block counts (an integer tree), and N = that count
template <bool MASKED>
__device__ __forceinline__ void lf_finalize_body(const LTerms &terms, const uint8_t *__restrict__ labeled,
                                                 int n_samples, int64_t pixels, const float *__restrict__ rec,
                                                 const unsigned long long *__restrict__ crec, int nrec, float *sums,
                                                 int64_t *counts, float *loss) {
    __shared__ double sh[3][256];
    __shared__ unsigned long long shc[MASKED ? 256 : 1];
    const int t = threadIdx.x;
    double total = 0;
    for (int k = 0; k < terms.n; ++k) {
        double acc[3] = {0, 0, 0};
        unsigned long long cacc = 0;
        for (int j = t; j < nrec; j += 256) {
            const lf4 r = *reinterpret_cast<const lf4 *>(rec + (size_t(k) * nrec + j) * LF_REC);
            acc[0] += r[0];
            acc[1] += r[1];
            acc[2] += r[2];
            if (MASKED) cacc += crec[size_t(k) * nrec + j];
        }
        sh[0][t] = acc[0];
        sh[1][t] = acc[1];
        sh[2][t] = acc[2];
        if (MASKED) shc[t] = cacc;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (t < off) {
                sh[0][t] += sh[0][t + off];
                sh[1][t] += sh[1][t + off];
                sh[2][t] += sh[2][t + off];
                if (MASKED) shc[t] += shc[t + off];
            }
            __syncthreads();
        }
        if (t == 0) {
            const scd_loss_term_t &T = terms.t[k];
            int cnt = 0;
            for (int s = 0; s < n_samples; ++s) cnt += lf_selected(T.select, labeled, s);
            const int cls = lf_class(T.kind);
            float *r = sums + k * LF_ROW;
            const float fI = float(sh[0][0]);
            const float fP = cls == LF_CLS_PTI ? float(sh[1][0]) : 0.f;
            const float fT = cls == LF_CLS_PTI ? float(sh[2][0]) : 0.f;
            const float fQ = cls == LF_CLS_IQ ? float(sh[1][0]) : 0.f;
            r[0] = fI;
            r[1] = fP;
            r[2] = fT;
            r[3] = fQ;
            r[4] = float(cnt);
            if (MASKED) {
                counts[k] = int64_t(shc[0]);
                total += double(T.coef) * lf_form_row_n(T.kind, r, double(int64_t(shc[0])), fI, fP, fT, fQ);
            } else {
                total += double(T.coef) * lf_form_row(T.kind, r, pixels, fI, fP, fT, fQ, float(cnt));
            }
        }
        __syncthreads();
    }
    if (t == 0) loss[0] = float(total);
}

__global__ __launch_bounds__(256) void loss_multi_finalize(LTerms terms, const uint8_t *__restrict__ labeled,
                                                           int n_samples, int64_t pixels,
                                                           const float *__restrict__ rec, int nrec, float *sums,
                                                           float *loss) {
    lf_finalize_body<false>(terms, labeled, n_samples, pixels, rec, nullptr, nrec, sums, nullptr, loss);
}

__global__ __launch_bounds__(256) void loss_masked_finalize(LTerms terms, const uint8_t *__restrict__ labeled,
                                                            int n_samples, int64_t pixels,
                                                            const float *__restrict__ rec,
                                                            const unsigned long long *__restrict__ crec, int nrec,
                                                            float *sums, int64_t *counts, float *loss) {
    lf_finalize_body<true>(terms, labeled, n_samples, pixels, rec, crec, nrec, sums, counts, loss);
}

// The exact-DataParallel loss: rows summed over the ranks (raw sums and sample counts add; the coefficient slots are
// overwritten here), re-formed exactly as loss_multi_finalize forms them from one device's sums.
__global__ void loss_multi_from_sums(LTerms terms, int64_t pixels, float *sums, float *loss) {
    if (threadIdx.x != 0) return;
    double total = 0;
    for (int k = 0; k < terms.n; ++k) {
        float *r = sums + k * LF_ROW;
        total += double(terms.t[k].coef) * lf_form_row(terms.t[k].kind, r, pixels, r[0], r[1], r[2], r[3], r[4]);
    }
    loss[0] = float(total);
}

// The masked form: N is the all-reduced int64 count of selected valid elements (an fp32 row cannot carry it exactly).
__global__ void loss_masked_from_sums(LTerms terms, float *sums, const int64_t *__restrict__ counts, float *loss) {
    if (threadIdx.x != 0) return;
    double total = 0;
    for (int k = 0; k < terms.n; ++k) {
        float *r = sums + k * LF_ROW;
        total += double(terms.t[k].coef) * lf_form_row_n(terms.t[k].kind, r, double(counts[k]), r[0], r[1], r[2], r[3]);
    }
    loss[0] = float(total);
}

// dL/dlogit (and dL/dtarget-logit) of one selected element
template <int CLS>
__device__ __forceinline__ void lf_grad(const scd_loss_term_t &T, float g, float a, float b, float c, float x,
                                        float tv, float &gl, float &gt) {
    const float q = T.soft_target ? lf_sigmoid(tv) : tv;
    const float dq = q * (1.f - q);  // only used for a soft target
    if (CLS == LF_CLS_BCE) {
        gl = g * a * (lf_sigmoid(x) - q);
        gt = -g * a * x * dq;
    } else if (CLS == LF_CLS_MSE) {
        const float p = lf_sigmoid(x);
        const float d = 2.f * g * a * ((T.sigmoid_input ? p : x) - q);
        gl = T.sigmoid_input ? d * (p * (1.f - p)) : d;
        gt = -d * dq;
    } else {  // every ratio kind
        const float p = lf_sigmoid(x);
        gl = g * (a + b * q + c * p) * (p * (1.f - p));
        gt = g * (a + b * p + c * q) * dq;
    }
}

// MASKED: a selected but invalid element always gets +0.0 (the gradient buffers are uninitialised), and its logit /
// target are not read
template <int CLS, bool MASKED>
__device__ __forceinline__ void lf_bwd_one(const scd_loss_term_t &T, const uint8_t *__restrict__ labeled,
                                           const uint8_t *__restrict__ valid, int64_t i, int64_t pixels, bool small,
                                           float g, float a, float b, float c) {
    if (T.select != 0 && !lf_selected(T.select, labeled, lf_sample(i, pixels, small))) {
        if (T.glogits && (T.zero_unselected & 1)) T.glogits[i] = 0.f;
        if (T.gtarget && (T.zero_unselected & 2)) T.gtarget[i] = 0.f;
        return;
    }
    if (MASKED && valid && valid[i] == 0) {
        if (T.glogits) T.glogits[i] = 0.f;
        if (T.gtarget) T.gtarget[i] = 0.f;
        return;
    }
    float gl, gt;
    lf_grad<CLS>(T, g, a, b, c, T.logits[i], T.target[i], gl, gt);
    if (T.glogits) T.glogits[i] = gl;
    if (T.gtarget) T.gtarget[i] = gt;
}

template <int CLS, bool MASKED>
__device__ __forceinline__ void lf_bwd_sweep(const scd_loss_term_t &T, const uint8_t *__restrict__ labeled,
                                             const uint8_t *__restrict__ valid, int64_t n, int64_t pixels, bool vec,
                                             float g, float a, float b, float c) {
    const bool small = n < (int64_t(1) << 31);
    const int64_t tid = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t nvec = vec ? n >> 2 : 0;
    for (int64_t v = tid; v < nvec; v += stride) {
        const int64_t i = v << 2;
        const int st = lf_vec_state(T.select, labeled, i, pixels, small);
        if (st == 2) {  // a sample boundary inside the vector: element by element
            for (int j = 0; j < 4; ++j) lf_bwd_one<CLS, MASKED>(T, labeled, valid, i + j, pixels, small, g, a, b, c);
            continue;
        }
        if (st == 0) {
            const lf4 z = {0.f, 0.f, 0.f, 0.f};
            if (T.glogits && (T.zero_unselected & 1)) *reinterpret_cast<lf4 *>(T.glogits + i) = z;
            if (T.gtarget && (T.zero_unselected & 2)) *reinterpret_cast<lf4 *>(T.gtarget + i) = z;
            continue;
        }
        uint32_t m = LF_ALL_VALID;
        if (MASKED) {
            if (valid) m = *reinterpret_cast<const uint32_t *>(valid + i);
            if (m == 0u) {  // nothing of this vector counts: zeros, and neither float load is issued
                const lf4 z = {0.f, 0.f, 0.f, 0.f};
                if (T.glogits) *reinterpret_cast<lf4 *>(T.glogits + i) = z;
                if (T.gtarget) *reinterpret_cast<lf4 *>(T.gtarget + i) = z;
                continue;
            }
        }
        const lf4 x = *reinterpret_cast<const lf4 *>(T.logits + i);
        const lf4 tv = *reinterpret_cast<const lf4 *>(T.target + i);
        lf4 gl, gt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float l, t;
            lf_grad<CLS>(T, g, a, b, c, x[j], tv[j], l, t);
            if (MASKED && !lf_valid_byte(m, j)) l = t = 0.f;  // a select: whatever the invalid element gave is dropped
            gl[j] = l;
            gt[j] = t;
        }
        if (T.glogits) *reinterpret_cast<lf4 *>(T.glogits + i) = gl;
        if (T.gtarget) *reinterpret_cast<lf4 *>(T.gtarget + i) = gt;
    }
    for (int64_t i = (nvec << 2) + tid; i < n; i += stride)
        lf_bwd_one<CLS, MASKED>(T, labeled, valid, i, pixels, small, g, a, b, c);
}

template <bool MASKED>
__device__ __forceinline__ void lf_bwd_body(const LTerms &terms, const uint8_t *__restrict__ labeled,
                                            const uint8_t *__restrict__ valid, int n_samples, int64_t pixels,
                                            unsigned vec_mask, const float *__restrict__ sums,
                                            const float *__restrict__ gloss) {
    const int k = blockIdx.y;
    const scd_loss_term_t T = terms.t[k];
    const float g = (gloss ? gloss[0] : 1.f) * T.coef;
    const float a = sums[k * LF_ROW + 5], b = sums[k * LF_ROW + 6], c = sums[k * LF_ROW + 7];
    const int64_t n = int64_t(n_samples) * pixels;
    const bool vec = (vec_mask >> k) & 1u;
    switch (lf_class(T.kind)) {
        case LF_CLS_BCE: lf_bwd_sweep<LF_CLS_BCE, MASKED>(T, labeled, valid, n, pixels, vec, g, a, b, c); break;
        case LF_CLS_MSE: lf_bwd_sweep<LF_CLS_MSE, MASKED>(T, labeled, valid, n, pixels, vec, g, a, b, c); break;
        default: lf_bwd_sweep<LF_CLS_IQ, MASKED>(T, labeled, valid, n, pixels, vec, g, a, b, c); break;
    }
}

__global__ __launch_bounds__(256) void loss_multi_bwd_kernel(LTerms terms, const uint8_t *__restrict__ labeled,
                                                             int n_samples, int64_t pixels, unsigned vec_mask,
                                                             const float *__restrict__ sums,
                                                             const float *__restrict__ gloss) {
    lf_bwd_body<false>(terms, labeled, nullptr, n_samples, pixels, vec_mask, sums, gloss);
}

__global__ __launch_bounds__(256) void loss_masked_bwd_kernel(LTerms terms, LMasks masks,
                                                              const uint8_t *__restrict__ labeled, int n_samples,
                                                              int64_t pixels, unsigned vec_mask,
                                                              const float *__restrict__ sums,
                                                              const float *__restrict__ gloss) {
    lf_bwd_body<true>(terms, labeled, masks.v[blockIdx.y], n_samples, pixels, vec_mask, sums, gloss);
}

// Host-side validation (before any GPU call); fills the by-value kernel argument and the per-term "16-byte loads
// allowed" mask (every pointer the term touches is 16-byte aligned).
static int lf_load(const scd_loss_term_t *terms, int n_terms, const uint8_t *labeled, LTerms &lt, unsigned &vec_mask,
                   const char *what) {
    if (!terms || n_terms < 1 || n_terms > LF_MAX) {
        set_error("%s: 1..%d terms", what, LF_MAX);
        return SCD_ERR_ARG;
    }
    lt.n = n_terms;
    vec_mask = 0;
    for (int k = 0; k < n_terms; ++k) {
        const scd_loss_term_t &T = terms[k];
        if (T.kind < 0 || T.kind >= SCD_LOSS_KIND_COUNT) {
            set_error("%s: term %d: unknown loss kind %d", what, k, T.kind);
            return SCD_ERR_ARG;
        }
        if (!T.logits || !T.target || T.select < 0 || T.select > 2) {
            set_error("%s: term %d: null logits / target or select outside 0..2", what, k);
            return SCD_ERR_ARG;
        }
        if (T.gtarget && !T.soft_target) {
            set_error("%s: term %d: gtarget only for a soft target", what, k);
            return SCD_ERR_ARG;
        }
        if (T.sigmoid_input && T.kind != SCD_LOSS_MSE) {
            set_error("%s: term %d: sigmoid_input only for SCD_LOSS_MSE", what, k);
            return SCD_ERR_ARG;
        }
        if (T.select != 0 && !labeled) {
            set_error("%s: term %d selects a subset but labeled is null", what, k);
            return SCD_ERR_ARG;
        }
        if (aligned16(T.logits) && aligned16(T.target) && aligned16(T.glogits) && aligned16(T.gtarget))
            vec_mask |= 1u << k;
        lt.t[k] = T;
    }
    return SCD_OK;
}

// The masked calls: lf_load, then the per-term mask pointers; a term keeps its 16-byte loads only where its mask
// pointer (if any) allows the 4-byte mask word that goes with them.
static int lf_load_masked(const scd_loss_term_t *terms, int n_terms, const uint8_t *labeled,
                          const uint8_t *const *valid, LTerms &lt, LMasks &lm, unsigned &vec_mask, const char *what) {
    SCD_TRY(lf_load(terms, n_terms, labeled, lt, vec_mask, what));
    if (!valid) {
        set_error("%s: null valid array (an unmasked term is a NULL entry of it)", what);
        return SCD_ERR_ARG;
    }
    for (int k = 0; k < LF_MAX; ++k) {
        lm.v[k] = k < n_terms ? valid[k] : nullptr;
        if ((reinterpret_cast<uintptr_t>(lm.v[k]) & 3u) != 0) vec_mask &= ~(1u << k);
    }
    return SCD_OK;
}

// the float partial records of n_terms terms (the masked calls keep their integer counts behind them)
static size_t lf_rec_bytes(int32_t n_terms) {
    return size_t(n_terms < 1 ? 1 : n_terms) * LF_BLOCKS * LF_REC * sizeof(float);
}

}  // namespace scd

using namespace scd;

extern "C" size_t scd_loss_multi_workspace_bytes(int32_t n_terms) { return lf_rec_bytes(n_terms); }

extern "C" int scd_loss_multi_fwd(const scd_loss_term_t *terms, int32_t n_terms, const uint8_t *labeled,
                                  int32_t n_samples, int64_t pixels, float *sums, float *loss, void *ws,
                                  size_t ws_bytes, scd_stream_t stream) {
    clear_error();
    LTerms lt;
    unsigned vec_mask;
    SCD_TRY(lf_load(terms, n_terms, labeled, lt, vec_mask, "loss_multi_fwd"));
    if (n_samples < 1 || pixels < 1 || !sums || !loss) {
        set_error("loss_multi_fwd: bad arguments");
        return SCD_ERR_ARG;
    }
    if (!ws || !aligned16(ws) || ws_bytes < scd_loss_multi_workspace_bytes(n_terms)) {
        set_error("loss_multi_fwd: workspace too small or not 16-byte aligned");
        return SCD_ERR_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    float *rec = static_cast<float *>(ws);
    // a function of the shape alone, so the summation order (and every bit of the result) is too
    const int64_t want = ((int64_t(n_samples) * pixels + 3) / 4 + 255) / 256;
    const int blocks = int(want < LF_BLOCKS ? want : LF_BLOCKS);
    hipLaunchKernelGGL(loss_multi_partial, dim3(blocks, n_terms), dim3(256), 0, s, lt, labeled, n_samples, pixels,
                       vec_mask, rec);
    hipLaunchKernelGGL(loss_multi_finalize, dim3(1), dim3(256), 0, s, lt, labeled, n_samples, pixels, rec, blocks, sums,
                       loss);
    return launch_status("scd_loss_multi_fwd");
}

extern "C" int scd_loss_multi_loss_from_sums(const scd_loss_term_t *terms, int32_t n_terms, int64_t pixels,
                                             float *sums, float *loss, scd_stream_t stream) {
    clear_error();
    LTerms lt;
    unsigned vec_mask;
    // the subsets were applied by the fwd call: no labeled array is read here
    static const uint8_t unused = 0;
    SCD_TRY(lf_load(terms, n_terms, &unused, lt, vec_mask, "loss_multi_loss_from_sums"));
    if (pixels < 1 || !sums || !loss) {
        set_error("loss_multi_loss_from_sums: bad arguments");
        return SCD_ERR_ARG;
    }
    hipLaunchKernelGGL(loss_multi_from_sums, dim3(1), dim3(64), 0, as_stream(stream), lt, pixels, sums, loss);
    return launch_status("scd_loss_multi_loss_from_sums");
}

extern "C" int scd_loss_multi_bwd(const scd_loss_term_t *terms, int32_t n_terms, const uint8_t *labeled,
                                  int32_t n_samples, int64_t pixels, const float *sums, const float *gloss,
                                  scd_stream_t stream) {
    clear_error();
    LTerms lt;
    unsigned vec_mask;
    SCD_TRY(lf_load(terms, n_terms, labeled, lt, vec_mask, "loss_multi_bwd"));
    if (n_samples < 1 || pixels < 1 || !sums) {
        set_error("loss_multi_bwd: bad arguments");
        return SCD_ERR_ARG;
    }
    const int64_t n = int64_t(n_samples) * pixels;
    int64_t blocks = ((n + 3) / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(loss_multi_bwd_kernel, dim3(unsigned(blocks), n_terms), dim3(256), 0, as_stream(stream), lt,
                       labeled, n_samples, pixels, vec_mask, sums, gloss);
    return launch_status("scd_loss_multi_bwd");
}

extern "C" size_t scd_loss_masked_workspace_bytes(int32_t n_terms) {
    return lf_rec_bytes(n_terms) + size_t(n_terms < 1 ? 1 : n_terms) * LF_BLOCKS * sizeof(unsigned long long);
}

extern "C" int scd_loss_masked_fwd(const scd_loss_term_t *terms, int32_t n_terms, const uint8_t *labeled,
                                   const uint8_t *const *valid, int32_t n_samples, int64_t pixels, float *sums,
                                   int64_t *counts, float *loss, void *ws, size_t ws_bytes, scd_stream_t stream) {
    clear_error();
    LTerms lt;
    LMasks lm;
    unsigned vec_mask;
    SCD_TRY(lf_load_masked(terms, n_terms, labeled, valid, lt, lm, vec_mask, "loss_masked_fwd"));
    if (!counts) {
        set_error("loss_masked_fwd: null counts");
        return SCD_ERR_ARG;
    }
    if (n_samples < 1 || pixels < 1 || !sums || !loss) {
        set_error("loss_masked_fwd: bad arguments");
        return SCD_ERR_ARG;
    }
    if (!ws || !aligned16(ws) || ws_bytes < scd_loss_masked_workspace_bytes(n_terms)) {
        set_error("loss_masked_fwd: workspace too small or not 16-byte aligned");
        return SCD_ERR_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    float *rec = static_cast<float *>(ws);
    auto *crec = reinterpret_cast<unsigned long long *>(static_cast<char *>(ws) + lf_rec_bytes(n_terms));
    // the grid of scd_loss_multi_fwd: a function of the shape alone, never of the mask
    const int64_t want = ((int64_t(n_samples) * pixels + 3) / 4 + 255) / 256;
    const int blocks = int(want < LF_BLOCKS ? want : LF_BLOCKS);
    hipLaunchKernelGGL(loss_masked_partial, dim3(blocks, n_terms), dim3(256), 0, s, lt, lm, labeled, n_samples, pixels,
                       vec_mask, rec, crec);
    hipLaunchKernelGGL(loss_masked_finalize, dim3(1), dim3(256), 0, s, lt, labeled, n_samples, pixels, rec, crec,
                       blocks, sums, counts, loss);
    return launch_status("scd_loss_masked_fwd");
}

extern "C" int scd_loss_masked_loss_from_sums(const scd_loss_term_t *terms, int32_t n_terms, float *sums,
                                              const int64_t *counts, float *loss, scd_stream_t stream) {
    clear_error();
    LTerms lt;
    unsigned vec_mask;
    static const uint8_t unused = 0;  // as scd_loss_multi_loss_from_sums: the subsets were applied by the fwd call
    SCD_TRY(lf_load(terms, n_terms, &unused, lt, vec_mask, "loss_masked_loss_from_sums"));
    if (!counts) {
        set_error("loss_masked_loss_from_sums: null counts");
        return SCD_ERR_ARG;
    }
    if (!sums || !loss) {
        set_error("loss_masked_loss_from_sums: bad arguments");
        return SCD_ERR_ARG;
    }
    hipLaunchKernelGGL(loss_masked_from_sums, dim3(1), dim3(64), 0, as_stream(stream), lt, sums, counts, loss);
    return launch_status("scd_loss_masked_loss_from_sums");
}

extern "C" int scd_loss_masked_bwd(const scd_loss_term_t *terms, int32_t n_terms, const uint8_t *labeled,
                                   const uint8_t *const *valid, int32_t n_samples, int64_t pixels, const float *sums,
                                   const float *gloss, scd_stream_t stream) {
    clear_error();
    LTerms lt;
    LMasks lm;
    unsigned vec_mask;
    SCD_TRY(lf_load_masked(terms, n_terms, labeled, valid, lt, lm, vec_mask, "loss_masked_bwd"));
    if (n_samples < 1 || pixels < 1 || !sums) {
        set_error("loss_masked_bwd: bad arguments");
        return SCD_ERR_ARG;
    }
    const int64_t n = int64_t(n_samples) * pixels;
    int64_t blocks = ((n + 3) / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(loss_masked_bwd_kernel, dim3(unsigned(blocks), n_terms), dim3(256), 0, as_stream(stream), lt, lm,
                       labeled, n_samples, pixels, vec_mask, sums, gloss);
    return launch_status("scd_loss_masked_bwd");
}
