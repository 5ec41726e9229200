// The parameter update on the device: the gradient norm of torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW's non-amsgrad step
// over ALL parameters in at most three launches, without a host read, bitwise reproducible from run to run (DESIGN.md 13;
// co_occ_amd/optim.py fills the tables).
//
// k_optim_sumsq (one fp64 partial per chunk) -> k_optim_clip_coef (partials added in a fixed order; norm and coefficient) ->
// k_optim_adamw (coefficient applied in registers, then the update) | k_optim_scale (the stand-alone clip).  In front of them, with a
// process group: k_optim_pack (every gradient / world into one arena) -> the all-reduce -> k_optim_flag_check; k_optim_unpack is
// the copy back.
// A chunk is OPT_CHUNK consecutive elements of one tensor, cut into groups of four: thread t of the workgroup owns groups t, t + 256,
// ...  That ownership is the same whatever the pointers' alignment -- an aligned chunk reads a group as one 16-byte load, any other
// chunk as four 4-byte loads, the tensor's last incomplete group always element by element -- so the order of every sum depends on the
// shapes alone.  No float atomics anywhere.
#include "common.h"

namespace {

typedef float op_f4 __attribute__((ext_vector_type(4)));

constexpr int OPT_CHUNK = 16384;             // elements per chunk = per workgroup: 16 groups of four per thread
constexpr int OPT_THREADS = 256;

struct OptSpan {
  int ti;                                    // tensor index, -1: nothing to do
  long long off;                             // first element of the chunk
  int n;                                     // elements in the chunk
};

// the chunk of this workgroup, bounds-checked against the tensor table: a table that disagrees with itself does nothing
__device__ __forceinline__ OptSpan opt_span(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                            const long long* __restrict__ chunks) {
  OptSpan s;
  const long long ti = chunks[2 * (size_t)blockIdx.x], off = chunks[2 * (size_t)blockIdx.x + 1];
  s.ti = -1; s.off = 0; s.n = 0;
  if (ti < 0 || ti >= ntensors) return s;
  const long long numel = tensors[ti].numel;
  if (off < 0 || off >= numel) return s;
  const long long left = numel - off;
  s.ti = (int)ti;
  s.off = off;
  s.n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  return s;
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements [base, base + 4) of a chunk of n elements: k of them exist (1..4)
__device__ __forceinline__ op_f4 load4(const float* __restrict__ x, int base, int k, bool vec) {
  op_f4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && k == 4) return *(const op_f4*)(x + base);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < k) v[e] = x[base + e];
  return v;
}

__device__ __forceinline__ void store4(float* __restrict__ x, int base, int k, bool vec, op_f4 v) {
  if (vec && k == 4) { *(op_f4*)(x + base) = v; return; }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < k) x[base + e] = v[e];
}

// ------------------------------------------------------------------ sum of squares of one chunk
__global__ __launch_bounds__(OPT_THREADS) void k_optim_sumsq(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                                              const long long* __restrict__ chunks, double* __restrict__ partials) {
  __shared__ double s_a[OPT_THREADS / 64];
  const int tid = threadIdx.x;
  const OptSpan s = opt_span(tensors, ntensors, chunks);
  double acc = 0;
  if (s.ti >= 0) {
    const float* g = tensors[s.ti].g + s.off;
    const bool vec = al16(g);
    const int ngroups = (s.n + 3) >> 2;
#pragma unroll 4
    for (int q = tid; q < ngroups; q += OPT_THREADS) {
      const int base = q << 2, k = s.n - base < 4 ? s.n - base : 4;
      const op_f4 v = load4(g, base, k, vec);                    // absent elements are 0 and add nothing
      acc += (double)v[0] * (double)v[0];
      acc += (double)v[1] * (double)v[1];
      acc += (double)v[2] * (double)v[2];
      acc += (double)v[3] * (double)v[3];
    }
  }
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
  if ((tid & 63) == 0) s_a[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, then the butterfly and the four waves in wave order
__global__ __launch_bounds__(OPT_THREADS) void k_optim_clip_coef(const double* __restrict__ partials, int nparts, float max_norm,
                                                                  double* __restrict__ norm64, float* __restrict__ norm32,
                                                                  float* __restrict__ coef) {
  __shared__ double s_a[OPT_THREADS / 64];
  const int tid = threadIdx.x;
  double a = 0;
  for (int k = tid; k < nparts; k += OPT_THREADS) a += partials[k];
  for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m);
  if ((tid & 63) == 0) s_a[tid >> 6] = a;
  __syncthreads();
  if (tid != 0) return;
  const double norm = sqrt(((s_a[0] + s_a[1]) + s_a[2]) + s_a[3]);
  const float nf = (float)norm;
  const float c = max_norm / (nf + 1e-6f);
  norm64[0] = norm;
  norm32[0] = nf;
  coef[0] = c > 1.f ? 1.f : c;                 // clamp(max = 1): a NaN stays a NaN
}

// ------------------------------------------------------------------ the update
// One element's step runs in fp64 registers from its fp32 loads, in torch's operation order, and rounds ONCE per stored value.  The
// same chain in fp32 rounds four times per step on the way to exp_avg_sq (the clipped gradient, its square, two products) and
// missed the float64 judge of tests/test_gpu_optim.py on single-element tensors, where no averaging hides an ulp (1.2 ulp after
// four steps against a budget of 1).  The hyper-parameters stay the host's float64 values, as torch's Python floats are.  Both
// kernels are bandwidth kernels: the fp64 arithmetic (one sqrt, one division per element) hides behind the 28 B / element.
struct OptScalars {
  double decay, w1, b2, w2, rsq2, eps, step;
};

__global__ __launch_bounds__(OPT_THREADS) void k_optim_adamw(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                                              const long long* __restrict__ chunks, const float* __restrict__ coef,
                                                              int write_grad) {
  const OptSpan s = opt_span(tensors, ntensors, chunks);
  if (s.ti < 0) return;
  const coocc_optim_tensor t = tensors[s.ti];
  float* __restrict__ p = t.p + s.off;
  float* __restrict__ g = t.g + s.off;
  float* __restrict__ m = t.exp_avg + s.off;
  float* __restrict__ v = t.exp_avg_sq + s.off;
  const bool vec = al16(p) && al16(g) && al16(m) && al16(v);
  const double cf = coef ? (double)coef[0] : 1.0;      // the fp32 coefficient of k_optim_clip_coef; g * 1.0 is g
  OptScalars c;
  c.decay = 1.0 - t.lr * t.weight_decay;
  c.w1 = 1.0 - t.beta1;
  c.b2 = t.beta2;
  c.w2 = 1.0 - t.beta2;
  c.rsq2 = 1.0 / sqrt(t.bias_correction2);
  c.eps = t.eps;
  c.step = t.lr / t.bias_correction1;
  const int ngroups = (s.n + 3) >> 2;
#pragma unroll 2
  for (int q = threadIdx.x; q < ngroups; q += OPT_THREADS) {
    const int base = q << 2, k = s.n - base < 4 ? s.n - base : 4;
    op_f4 pv = load4(p, base, k, vec), gv = load4(g, base, k, vec), mv = load4(m, base, k, vec), vv = load4(v, base, k, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double ge = (double)gv[e] * cf;              // exact: the product of two fp32 values
      const double pe = (double)pv[e] * c.decay;                             // p *= 1 - lr wd
      const double me = (double)mv[e] + (ge - (double)mv[e]) * c.w1;         // m += (g - m)(1 - b1)
      const double ve = (double)vv[e] * c.b2 + ge * ge * c.w2;               // v = v b2 + g g (1 - b2)
      const double denom = sqrt(ve) * c.rsq2 + c.eps;                        // sqrt(v) / sqrt(bc2) + eps
      pv[e] = (float)(pe - c.step * (me / denom));                           // p -= (lr / bc1) m / denom
      gv[e] = (float)ge;                                 // what the fp32 product g * coef rounds to
      mv[e] = (float)me;
      vv[e] = (float)ve;
    }
    store4(p, base, k, vec, pv);
    store4(m, base, k, vec, mv);
    store4(v, base, k, vec, vv);
    if (write_grad) store4(g, base, k, vec, gv);
  }
}

__global__ __launch_bounds__(OPT_THREADS) void k_optim_scale(const coocc_optim_tensor* __restrict__ tensors,
                                                                                int ntensors, const long long* __restrict__ chunks,
                                                                                const float* __restrict__ coef) {
  const float cf = coef[0];
  if (cf == 1.f) return;                       // the clip is inactive: the gradients keep their bits
  const OptSpan s = opt_span(tensors, ntensors, chunks);
  if (s.ti < 0) return;
  float* __restrict__ g = tensors[s.ti].g + s.off;
  const bool vec = al16(g);
  const int ngroups = (s.n + 3) >> 2;
#pragma unroll 4
  for (int q = threadIdx.x; q < ngroups; q += OPT_THREADS) {
    const int base = q << 2, k = s.n - base < 4 ? s.n - base : 4;
    op_f4 gv = load4(g, base, k, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = gv[e] * cf;
    store4(g, base, k, vec, gv);
  }
}

// ------------------------------------------------------------------ data-parallel gradient averaging
// The arena is one fp32 buffer: a header of one float per layout tensor, then one segment per tensor at a multiple of four elements.
// In the tables of these kernels one of the two pointers of an entry is the tensor's arena segment: p for pack (g is the source, NULL:
// this rank has no gradient), g for unpack (p is the destination).  The arena side is 16-byte aligned by construction; the other side
// picks 16- or 4-byte accesses by its pointer.  The padding between segments is never written.
__global__ __launch_bounds__(OPT_THREADS) void k_optim_pack(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                                             const long long* __restrict__ chunks, float* __restrict__ header,
                                                             float world) {
  const OptSpan s = opt_span(tensors, ntensors, chunks);
  if (s.ti < 0) return;
  const float* src = tensors[s.ti].g;
  float* __restrict__ dst = tensors[s.ti].p + s.off;
  if (s.off == 0 && threadIdx.x == 0) header[s.ti] = src ? 1.f : 0.f;       // the presence flag: never divided
  const float* __restrict__ g = src ? src + s.off : nullptr;
  const bool vec = g && al16(g);
  const int ngroups = (s.n + 3) >> 2;
#pragma unroll 4
  for (int q = threadIdx.x; q < ngroups; q += OPT_THREADS) {
    const int base = q << 2, k = s.n - base < 4 ? s.n - base : 4;
    op_f4 gv = {0.f, 0.f, 0.f, 0.f};
    if (g) {
      gv = load4(g, base, k, vec);
      if (world != 1.f) {                        // world == 1 copies the bits
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = __fdiv_rn(gv[e], world);        // correctly rounded: DDP divides
      }
    }
    store4(dst, base, k, true, gv);
  }
}

__global__ __launch_bounds__(OPT_THREADS) void k_optim_unpack(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                                               const long long* __restrict__ chunks) {
  const OptSpan s = opt_span(tensors, ntensors, chunks);
  if (s.ti < 0) return;
  const float* __restrict__ src = tensors[s.ti].g + s.off;
  float* __restrict__ dst = tensors[s.ti].p + s.off;
  const bool vec = al16(dst);
  const int ngroups = (s.n + 3) >> 2;
#pragma unroll 4
  for (int q = threadIdx.x; q < ngroups; q += OPT_THREADS) {
    const int base = q << 2, k = s.n - base < 4 ? s.n - base : 4;
    store4(dst, base, k, vec, load4(src, base, k, true));
  }
}

// one workgroup over pack's tensor table after the reduce: header[i] is the number of ranks that had a gradient for tensor i, a small
// integer and exact in fp32; every rank presenting the same set means world where this rank had one and 0 where it had none.  The count
// of the others is ADDED to the sticky word by one thread (launches on a stream are ordered: no atomic needed).
__global__ __launch_bounds__(OPT_THREADS) void k_optim_flag_check(const coocc_optim_tensor* __restrict__ tensors, int ntensors,
                                                                   const float* __restrict__ header, float world,
                                                                   int* __restrict__ sticky) {
  __shared__ int s_a[OPT_THREADS / 64];
  const int tid = threadIdx.x;
  int bad = 0;
  for (int i = tid; i < ntensors; i += OPT_THREADS) {
    const float want = tensors[i].g ? world : 0.f;
    bad += header[i] != want ? 1 : 0;            // a NaN counts
  }
  for (int m = 32; m > 0; m >>= 1) bad += __shfl_xor(bad, m);
  if ((tid & 63) == 0) s_a[tid >> 6] = bad;
  __syncthreads();
  if (tid == 0) sticky[0] += s_a[0] + s_a[1] + s_a[2] + s_a[3];
}

// what the host can check of the tables before a launch: the tensor table's host copy gives every numel and pointer, and with them the
// chunk count the chunk table must have.  Returns nullptr or the complaint.
static const char* opt_check(const coocc_optim_tensor* tensors, const coocc_optim_tensor* th, int ntensors, const int64_t* chunks,
                             int nchunks, bool moments) {
  if (!tensors || !th || !chunks) return "null table";
  if (ntensors <= 0 || nchunks <= 0) return "ntensors and nchunks must be positive";
  int64_t want = 0;
  for (int i = 0; i < ntensors; ++i) {
    const coocc_optim_tensor& t = th[i];
    if (t.numel <= 0) return "a tensor with numel <= 0";
    if (!t.g || ((uintptr_t)t.g & 3)) return "a null or misaligned gradient pointer";
    if (moments && (!t.p || !t.exp_avg || !t.exp_avg_sq || (((uintptr_t)t.p | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 3)))
      return "a null or misaligned parameter or moment pointer";
    want += (t.numel + OPT_CHUNK - 1) / OPT_CHUNK;
  }
  if (want != (int64_t)nchunks) return "nchunks is not the chunk count of the tensor table";
  return nullptr;
}

// the same for the tables of pack (the arena side is p, the tensor side g and may be NULL) and unpack (the arena side is g): every
// segment 16-byte aligned and wholly inside [arena + header, arena + arena_numel), segments in ascending order without overlap
static const char* opt_check_arena(const coocc_optim_tensor* tensors, const coocc_optim_tensor* th, int ntensors, const int64_t* chunks,
                                   int nchunks, const float* arena, int64_t arena_numel, int64_t header, bool pack) {
  if (!tensors || !th || !chunks) return "null table";
  if (ntensors <= 0 || nchunks <= 0) return "ntensors and nchunks must be positive";
  if (!arena || ((uintptr_t)arena & 15)) return "a null or misaligned arena";
  if (header < 0 || arena_numel < header) return "an arena shorter than its header";
  const uintptr_t lo = (uintptr_t)arena + 4 * (uintptr_t)header, hi = (uintptr_t)arena + 4 * (uintptr_t)arena_numel;
  uintptr_t prev = lo;
  int64_t want = 0;
  for (int i = 0; i < ntensors; ++i) {
    const coocc_optim_tensor& t = th[i];
    if (t.numel <= 0) return "a tensor with numel <= 0";
    const uintptr_t seg = (uintptr_t)(pack ? t.p : t.g), other = (uintptr_t)(pack ? t.g : t.p);
    if (!seg || (seg & 15)) return "an arena segment that is null or not 16-byte aligned";
    if (seg < prev || seg > hi || (uint64_t)t.numel > (hi - seg) / 4) return "an arena segment outside the arena or not in ascending order";
    prev = seg + 4 * (uintptr_t)t.numel;
    if (pack ? (other & 3) != 0 : (!other || (other & 3))) return pack ? "a misaligned gradient pointer" : "a null or misaligned destination";
    want += (t.numel + OPT_CHUNK - 1) / OPT_CHUNK;
  }
  if (want != (int64_t)nchunks) return "nchunks is not the chunk count of the tensor table";
  return nullptr;
}

}  // namespace

extern "C" int coocc_optim_chunk(void) { return OPT_CHUNK; }

extern "C" int coocc_optim_pack(const coocc_optim_tensor* tensors, const coocc_optim_tensor* tensors_host, int ntensors,
                                const int64_t* chunks, int nchunks, float* arena, int64_t arena_numel, int world, void* stream) {
  const char* why = opt_check_arena(tensors, tensors_host, ntensors, chunks, nchunks, arena, arena_numel, ntensors, true);
  COOCC_CHECK_ARG(!why, "optim_pack: %s (ntensors=%d nchunks=%d)", why, ntensors, nchunks);
  COOCC_CHECK_ARG(world >= 1 && world <= (1 << 24), "optim_pack: world = %d (1 .. 2^24)", world);
  hipLaunchKernelGGL(k_optim_pack, dim3(nchunks), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors, (const long long*)chunks,
                     arena, (float)world);
  COOCC_LAUNCH_CHECK("k_optim_pack");
  return COOCC_OK;
}

extern "C" int coocc_optim_unpack(const coocc_optim_tensor* tensors, const coocc_optim_tensor* tensors_host, int ntensors,
                                  const int64_t* chunks, int nchunks, const float* arena, int64_t arena_numel, void* stream) {
  const char* why = opt_check_arena(tensors, tensors_host, ntensors, chunks, nchunks, arena, arena_numel, 0, false);
  COOCC_CHECK_ARG(!why, "optim_unpack: %s (ntensors=%d nchunks=%d)", why, ntensors, nchunks);
  hipLaunchKernelGGL(k_optim_unpack, dim3(nchunks), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors,
                     (const long long*)chunks);
  COOCC_LAUNCH_CHECK("k_optim_unpack");
  return COOCC_OK;
}

extern "C" int coocc_optim_flag_check(const coocc_optim_tensor* tensors, int ntensors, const float* header, int world, int* sticky,
                                      void* stream) {
  COOCC_CHECK_ARG(tensors && header && sticky, "optim_flag_check: null pointer");
  COOCC_CHECK_ARG(ntensors > 0, "optim_flag_check: ntensors = %d (positive)", ntensors);
  COOCC_CHECK_ARG(world >= 1 && world <= (1 << 24), "optim_flag_check: world = %d (1 .. 2^24)", world);
  hipLaunchKernelGGL(k_optim_flag_check, dim3(1), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors, header, (float)world,
                     sticky);
  COOCC_LAUNCH_CHECK("k_optim_flag_check");
  return COOCC_OK;
}

extern "C" int coocc_optim_sumsq(const coocc_optim_tensor* tensors, const coocc_optim_tensor* tensors_host, int ntensors,
                                 const int64_t* chunks, int nchunks, double* partials, void* stream) {
  const char* why = opt_check(tensors, tensors_host, ntensors, chunks, nchunks, false);
  COOCC_CHECK_ARG(!why, "optim_sumsq: %s (ntensors=%d nchunks=%d)", why, ntensors, nchunks);
  COOCC_CHECK_ARG(partials, "optim_sumsq: null partials");
  hipLaunchKernelGGL(k_optim_sumsq, dim3(nchunks), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors,
                     (const long long*)chunks, partials);
  COOCC_LAUNCH_CHECK("k_optim_sumsq");
  return COOCC_OK;
}

extern "C" int coocc_optim_clip_coef(const double* partials, int nchunks, float max_norm, double* norm64, float* norm32, float* coef,
                                     void* stream) {
  COOCC_CHECK_ARG(partials && norm64 && norm32 && coef, "optim_clip_coef: null pointer");
  COOCC_CHECK_ARG(nchunks > 0, "optim_clip_coef: nchunks = %d (at least one partial)", nchunks);
  COOCC_CHECK_ARG(max_norm > 0.f, "optim_clip_coef: max_norm = %g (positive)", (double)max_norm);
  hipLaunchKernelGGL(k_optim_clip_coef, dim3(1), dim3(OPT_THREADS), 0, as_stream(stream), partials, nchunks, max_norm, norm64, norm32,
                     coef);
  COOCC_LAUNCH_CHECK("k_optim_clip_coef");
  return COOCC_OK;
}

extern "C" int coocc_optim_adamw(const coocc_optim_tensor* tensors, const coocc_optim_tensor* tensors_host, int ntensors,
                                 const int64_t* chunks, int nchunks, const float* coef, int write_grad, void* stream) {
  const char* why = opt_check(tensors, tensors_host, ntensors, chunks, nchunks, true);
  COOCC_CHECK_ARG(!why, "optim_adamw: %s (ntensors=%d nchunks=%d)", why, ntensors, nchunks);
  for (int i = 0; i < ntensors; ++i) {
    const coocc_optim_tensor& t = tensors_host[i];
    COOCC_CHECK_ARG(t.bias_correction1 > 0.0 && t.bias_correction2 > 0.0,
                    "optim_adamw: tensor %d has bias corrections %g, %g (positive: its step count is at least 1)", i,
                    t.bias_correction1, t.bias_correction2);
  }
  hipLaunchKernelGGL(k_optim_adamw, dim3(nchunks), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors,
                     (const long long*)chunks, coef, write_grad);
  COOCC_LAUNCH_CHECK("k_optim_adamw");
  return COOCC_OK;
}

extern "C" int coocc_optim_scale(const coocc_optim_tensor* tensors, const coocc_optim_tensor* tensors_host, int ntensors,
                                 const int64_t* chunks, int nchunks, const float* coef, void* stream) {
  const char* why = opt_check(tensors, tensors_host, ntensors, chunks, nchunks, false);
  COOCC_CHECK_ARG(!why, "optim_scale: %s (ntensors=%d nchunks=%d)", why, ntensors, nchunks);
  COOCC_CHECK_ARG(coef, "optim_scale: null coef");
  hipLaunchKernelGGL(k_optim_scale, dim3(nchunks), dim3(OPT_THREADS), 0, as_stream(stream), tensors, ntensors,
                     (const long long*)chunks, coef);
  COOCC_LAUNCH_CHECK("k_optim_scale");
  return COOCC_OK;
}
