// fidelity.hip -- improved precision / recall of two feature sets on the device (include/medfusion_hip.h, MfFidelityDesc): squared distances between
// the rows of two fp32 feature banks on the fp32 matrix cores, and three things done with a 128 x 128 tile of them while it is still in the
// accumulators: stored (mf_feat_sqdist_f32), merged into every row's ascending list of its 16 smallest (the k-NN radii), or compared with the
// rows' radii (manifold membership).  The N x M matrix is never written by the last two.
// The neighbour family (README "Neighbours") adds two epilogues on the same tile -- every query row's 16 smallest pairs (d2, reference index) across
// TWO banks as 64-bit keys in lexicographic order (mf_nn_partial_f32 / mf_nn_finish_f32), and the COUNT of the balls a query lies in
// (mf_manifold_count_*) -- and pair_sqdist_kernel, the exact distance of listed pairs by differences, the sum in fp64 (mf_pair_sqdist_f32).
// The kernel distances (README "Kernel distances", MfKernelSumDesc) add two more: the fp64 SUM of a kernel k(x, y) -- polynomial or Gaussian -- over
// a tile of a pair of row subsets gathered through index lists (mf_ksum_partial_f32 / mf_ksum_finish_f64: KID and the unbiased MMD^2), and k stored
// as a matrix (mf_feat_kernel_f32).
//
// The definition (README "Fidelity"): xt = fl32(x - c) with the pivot c, n(x) = the fp64 sum of xt_k^2 rounded to fp32,
//   d2(x, y) = max(0, fl32(fl32(n(x) + n(y)) - 2 dot(xt, yt))),   dot = ONE fp32 fmaf chain over k ascending (v_mfma_f32_32x32x2_f32 is that chain).
// There is no split-K: the bits of d2(i, j) depend on the two rows and the pivot only -- not on the tile, the grid, N, M or the rows' places in
// their banks -- and d2(i, j) of (x, y) is d2(j, i) of (y, x).  No atomics anywhere: the column / row splits of the k-NN and manifold launches write
// partial lists / flags to a workspace, and a finish launch merges them in ascending split order.
// The structure: ONE K loop (tile_dot, with its loader load_chunk) over two row sources -- BankRows, a contiguous bank, or GatheredRows, a subset
// through an index list; ONE walk of the accumulators (for_each_acc) that hands every dot product to an epilogue, which makes it a value (d2_value,
// kernel_value); ONE body per kind of epilogue -- store_tile (d2 or k as a matrix), list_partial (the ValueList or the KeyList policy),
// manifold_partial (flags or counts) -- under kernels that keep their own names.  Every promise above is a statement about that one loop.
// Built without packed fp32 like metrics.hip (medfusion_amd/build.py): the staging subtraction and the epilogues are plain fp32 VALU work.
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int TM = 128;                 // rows of bank A and rows of bank B per workgroup: a TM x TM tile of d2
constexpr int BK = 32;                  // k per staged chunk
constexpr int LDK = BK + 4;             // a staged row: +4 floats, so that the sixteen lanes of a ds_read_b128 group hit sixteen different 16-byte slots
constexpr int OPER = TM * LDK;          // one operand's chunk
constexpr int BUF = 2 * OPER;           // A and B of one chunk
constexpr int STAGE = 2 * BUF;          // two chunks: 18432 floats
constexpr int LDT = TM + 1;             // a row of the d2 tile when it goes through LDS (the k-NN selection reads it row by thread)
constexpr int LIST = MF_FIDELITY_LIST;  // 16 values per row and split
constexpr int SMEM = STAGE + 2 * TM;    // + the A rows' norms and radii

// A row source tells thread t where the q-th of the four rows it stages in every chunk (the tile's row (t + 256 q) / 8) lies, and whether that row
// exists: the address is always inside the bank, a row past the end takes the last one's address and is masked.
// BankRows: rows r0 .. of a contiguous bank.  The address is formed from the three scalars at every use: nothing per row is held in registers
// across the K loop (the list kernels have none to spare).
struct BankRows {
  const float* __restrict__ bank;
  int rows, r0;
  __device__ __forceinline__ const float* row(int q, int t, int D, bool& in) const {
    const int r = r0 + ((t + 256 * q) >> 3);
    in = r < rows;
    return bank + (long)min(r, rows - 1) * D;
  }
};

// GatheredRows: rows of a subset, looked up ONCE per tile by gather_rows() below and held as four addresses and four flags
struct GatheredRows {
  const float* ptr[4];
  bool in[4];
  __device__ __forceinline__ const float* row(int q, int, int, bool& in_q) const {
    in_q = in[q];
    return ptr[q];
  }
};

// row r of a subset of `count` rows as a row of the bank: gathered through `list` (null: the identity), clamped into the subset before the
// list is read and into the bank before the index is ever used as an address
__device__ __forceinline__ int gather_index(const int* __restrict__ list, int r, int count, int rows) {
  const int rc = min(r, count - 1);
  return list ? min(max(list[rc], 0), rows - 1) : rc;
}

__device__ __forceinline__ GatheredRows gather_rows(const float* __restrict__ bank, int rows, const int* __restrict__ list, int count, int r0, int D, int t) {
  GatheredRows g;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + ((t + 256 * q) >> 3);
    g.in[q] = r < count;
    g.ptr[q] = bank + (long)gather_index(list, r, count, rows) * D;
  }
  return g;
}

// One chunk of one operand, global -> registers: 128 rows x 32 k as 1024 groups of four consecutive k, four groups per thread.  The pivot is
// subtracted here; zeros past the last row and past D (a zero row adds fma(0, 0, acc) = acc to the chain: nothing).  V = 4: sixteen-byte loads
// (D % 4 == 0: a group is inside or outside as a whole); V = 1: element by element.  The same values either way.  Every load is issued
// UNCONDITIONALLY from an address clamped into the bank and masked afterwards by a select: a branch around a load makes the compiler wait for
// each load before the next one, eight memory round trips per chunk instead of one.
template <int V, class Rows>
__device__ __forceinline__ void load_chunk(const Rows& src, int D, int k0, const float* __restrict__ pivot, int t, f32x4 (&reg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + ((t + 256 * q) & 7) * 4;
    bool row_in;
    const float* __restrict__ p = src.row(q, t, D, row_in);
    f32x4 v;
    if (V == 4) {
      const int kc = min(k, D - 4);
      const f32x4 d = *reinterpret_cast<const f32x4*>(p + kc) - *reinterpret_cast<const f32x4*>(pivot + kc);
      const bool in = row_in && k < D;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = in ? d[e] : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kc = min(k + e, D - 1);
        const float d = p[kc] - pivot[kc];
        v[e] = (row_in && k + e < D) ? d : 0.f;
      }
    }
    reg[q] = v;
  }
}

// registers -> LDS.  Inside every group of eight k the staged order is k = 0 2 4 6 1 3 5 7: lane (row, half h) of the wave then reads ITS four
// operands of the next four matrix instructions -- k = 2t + h, t = 0 .. 3 -- as one 16-byte read, and instruction t covers k = 2t, 2t + 1: ascending.
__device__ __forceinline__ void store_chunk(float* __restrict__ dst, int t, const f32x4 (&reg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = t + 256 * q, row = idx >> 3, c4 = idx & 7;
    float* d = dst + row * LDK + 8 * (c4 >> 1) + 2 * (c4 & 1);
    *reinterpret_cast<f32x2*>(d) = f32x2{reg[q][0], reg[q][2]};
    *reinterpret_cast<f32x2*>(d + 4) = f32x2{reg[q][1], reg[q][3]};
  }
}

// acc[m][n] = the dot products of rows wr 64 + m 32 + (0 .. 31) of source A with rows wc 64 + n 32 + (0 .. 31) of source B, wave (wr, wc) of the
// 2 x 2 waves.  THE K loop of this unit: every d2 and every k is a value of this one chain, whatever the sources are.
// K goes through LDS in chunks of BK, two buffers: the next chunk's global loads are in flight while this one is multiplied, and are written to
// the other buffer behind it -- one barrier per chunk.  Enters with a barrier (smem may still be read as the previous tile's d2) and leaves with
// one (smem is free again).
template <int V, class RowsA, class RowsB>
__device__ __forceinline__ void tile_dot(const RowsA& A, const RowsB& B, int D, const float* __restrict__ pivot, float* __restrict__ smem,
                                         f32x16 (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1, j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  f32x4 ra[4], rb[4];
  const int chunks = (D + BK - 1) / BK;
  load_chunk<V>(A, D, 0, pivot, t, ra);
  load_chunk<V>(B, D, 0, pivot, t, rb);
  __syncthreads();
  store_chunk(smem, t, ra);
  store_chunk(smem + OPER, t, rb);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    const float* cur = smem + (c & 1) * BUF;
    const bool more = c + 1 < chunks;
    if (more) {
      load_chunk<V>(A, D, (c + 1) * BK, pivot, t, ra);
      load_chunk<V>(B, D, (c + 1) * BK, pivot, t, rb);
    }
    const float* As = cur + (wr * 64 + j) * LDK + 4 * h;
    const float* Bs = cur + OPER + (wc * 64 + j) * LDK + 4 * h;
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
      const f32x4 fa0 = *reinterpret_cast<const f32x4*>(As + 8 * g), fa1 = *reinterpret_cast<const f32x4*>(As + 32 * LDK + 8 * g);
      const f32x4 fb0 = *reinterpret_cast<const f32x4*>(Bs + 8 * g), fb1 = *reinterpret_cast<const f32x4*>(Bs + 32 * LDK + 8 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[s], fb0[s], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[s], fb1[s], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[s], fb0[s], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[s], fb1[s], acc[1][1], 0, 0, 0);
      }
    }
    if (more) {
      float* nxt = smem + ((c + 1) & 1) * BUF;
      store_chunk(nxt, t, ra);
      store_chunk(nxt + OPER, t, rb);
    }
    __syncthreads();
  }
}

// Every element this lane holds, handed to f(local row, local column, n, dot): n tells which of the lane's two columns it is.  The one place that
// knows the accumulator layout of the 32 x 32 instruction: the lane's column is lane & 31, register r is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <class F>
__device__ __forceinline__ void for_each_acc(const f32x16 (&acc)[2][2], F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1, j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) f(wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, wc * 64 + n * 32 + j, n, acc[m][n][r]);
}

// the value functions of an element: its two rows' norms and their dot product in, d2 or k out
__device__ __forceinline__ float d2_value(float na, float nb, float dot) {
  const float s = na + nb;
  return fmaxf(s - 2.f * dot, 0.f);
}

// The kernel distances (README "Kernel distances", MfKernelSumDesc): poly: v = fmaf(gamma, dot(x, y), c0), k = v, v v, (v v) v, (v v)(v v) for
// degree 1 .. 4, every product rounded to fp32 (the unit is built with -ffp-contract=off); the callers pass a pivot of zeros: x - 0 is x bit for
// bit.  rbf: k = expf(fl32(-gamma d2)) of d2_value.  Nothing else enters: the bits of k(i, j) depend on the two rows, the pivot and the scalars,
// and k(i, j) = k(j, i) (the fmaf chain's products and the sum of the two norms commute).
struct KernelParams {
  int kind, degree;
  float gamma, coef0;
};

__device__ __forceinline__ float kernel_value(const KernelParams& kp, float na, float nb, float dot) {
  if (kp.kind == MF_KERNEL_RBF) return expf(-(kp.gamma * d2_value(na, nb, dot)));
  const float v = fmaf(kp.gamma, dot, kp.coef0);
  const float v2 = v * v;
  return kp.degree == 1 ? v : kp.degree == 2 ? v2 : kp.degree == 3 ? v2 * v : v2 * v2;
}

// the norms of the lane's two columns; zeros past the end, and for a kernel that needs no norms (nb null)
__device__ __forceinline__ void column_norms(const float* __restrict__ nb, int NB, int b0, float (&out)[2]) {
  const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int jg = b0 + wc * 64 + n * 32 + (lane & 31);
    out[n] = (nb && jg < NB) ? nb[jg] : 0.f;
  }
}

// ---- epilogue 1: the tile's values stored as a matrix: out[i][j] = value(i, j, n(x_i), n(y_j), dot)
template <int V, class Value>
__device__ __forceinline__ void store_tile(const float* __restrict__ x, const float* __restrict__ nx, const float* __restrict__ y,
                                           const float* __restrict__ ny, const float* __restrict__ pivot, float* __restrict__ out, int N, int M, int D,
                                           int col_tiles, Value value) {
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  const int t = threadIdx.x;
  const int rt = blockIdx.x / col_tiles, ct = blockIdx.x - rt * col_tiles;
  const int a0 = rt * TM, b0 = ct * TM;
  float* na = smem + STAGE;
  if (t < TM) na[t] = (nx && a0 + t < N) ? nx[a0 + t] : 0.f;
  f32x16 acc[2][2];
  tile_dot<V>(BankRows{x, N, a0}, BankRows{y, M, b0}, D, pivot, smem, acc);
  float nb[2];
  column_norms(ny, M, b0, nb);
  for_each_acc(acc, [&](int il, int jl, int n, float dot) {
    const int ig = a0 + il, jg = b0 + jl;
    if (ig < N && jg < M) out[(long)ig * M + jg] = value(ig, jg, na[il], nb[n], dot);
  });
}

// d2; with same_bank the diagonal is exactly 0
template <int V>
__global__ __launch_bounds__(256) void sqdist_kernel(const float* __restrict__ x, const float* __restrict__ nx, const float* __restrict__ y,
                                                     const float* __restrict__ ny, const float* __restrict__ pivot, float* __restrict__ out, int N, int M,
                                                     int D, int col_tiles, int same_bank) {
  store_tile<V>(x, nx, y, ny, pivot, out, N, M, D, col_tiles, [=](int ig, int jg, float na, float nb, float dot) {
    const float d = d2_value(na, nb, dot);
    return (same_bank && ig == jg) ? 0.f : d;
  });
}

// k (for tests and kernel_matrix()); the polynomial kernel's norms may be null
template <int V>
__global__ __launch_bounds__(256) void kernel_matrix_kernel(const float* __restrict__ x, const float* __restrict__ nx, const float* __restrict__ y,
                                                            const float* __restrict__ ny, const float* __restrict__ pivot, float* __restrict__ out, int N,
                                                            int M, int D, int col_tiles, KernelParams kp) {
  store_tile<V>(x, nx, y, ny, pivot, out, N, M, D, col_tiles, [=](int, int, float na, float nb, float dot) { return kernel_value(kp, na, nb, dot); });
}

// ---- epilogue 2: every row's ascending list of its 16 smallest entries over the column tiles of split blockIdx.y
// An entry is a value -- d2 alone, float order: ties cannot matter (the k-NN radii) -- or a key: the pair (d2, j) as 64 bits, the bits of d2 high and
// the reference index j low (the neighbour search).  d2 >= 0, so unsigned order of the keys is the lexicographic order (d2 as a float, then the
// smaller j).  The indices are unique, so that order is total and the k smallest keys of a row are a SET: no tile, split count or order of merging
// can change them.  -0 becomes +0 before packing (fmaxf(-0, 0) may return either; the raw bits of -0 would sort last).  An empty slot is
// (+inf, -1): above every real entry, a real +inf included.
typedef unsigned long long nnkey;
constexpr nnkey NN_EMPTY = 0x7F800000FFFFFFFFull;

__device__ __forceinline__ nnkey nn_key(float d, int j) {
  unsigned b = __float_as_uint(d);
  b = b == 0x80000000u ? 0u : b;
  return ((nnkey)b << 32) | (unsigned)j;
}

__device__ __forceinline__ float list_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float list_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ nnkey list_min(nnkey a, nnkey b) { return a < b ? a : b; }
__device__ __forceinline__ nnkey list_max(nnkey a, nnkey b) { return a < b ? b : a; }

// v goes in where it belongs, the largest falls out
template <class E>
__device__ __forceinline__ void list_insert(E (&l)[LIST], E v) {
  if (v < l[LIST - 1]) {
#pragma unroll
    for (int p = 0; p < LIST; ++p) {
      const E lo = list_min(l[p], v);
      v = list_max(l[p], v);
      l[p] = lo;
    }
  }
}

// What the two kinds of list do differently.  staged: what the tile in LDS holds for query row ig and reference row jg; takes: whether column j
// is inserted at all; WORDS: a row of the hand-over between the two halves, in 4-byte words (odd: no bank conflicts); store: the row's list to
// the workspace.
struct ValueList {      // the bank against itself: the row itself counts, as exactly 0; a column past the end is +inf
  typedef float Entry;
  static constexpr int WORDS = LIST + 1;
  static __device__ __forceinline__ Entry empty() { return INFINITY; }
  static __device__ __forceinline__ float staged(int ig, int jg, int refs, float d) { return jg >= refs ? INFINITY : (ig == jg ? 0.f : d); }
  static __device__ __forceinline__ bool takes(int, int, int) { return true; }
  static __device__ __forceinline__ Entry entry(float d, int) { return d; }
  static __device__ __forceinline__ void put(float* w, int p, Entry e) { w[p] = e; }
  static __device__ __forceinline__ Entry get(const float* w, int p) { return w[p]; }
  static __device__ __forceinline__ void store(Entry* __restrict__ o, const Entry (&l)[LIST]) {
#pragma unroll
    for (int p = 0; p < LIST; p += 4) *reinterpret_cast<f32x4*>(o + p) = f32x4{l[p], l[p + 1], l[p + 2], l[p + 3]};
  }
};

struct KeyList {        // a column past the end of the bank is never inserted; with exclude_self the entry j == i is skipped BY INDEX: another
  typedef nnkey Entry;  // row with the same features stays a neighbour at 0
  static constexpr int WORDS = 2 * LIST + 1;      // (low, high, low, high, ...)
  static __device__ __forceinline__ Entry empty() { return NN_EMPTY; }
  static __device__ __forceinline__ float staged(int, int, int, float d) { return d; }
  static __device__ __forceinline__ bool takes(int j, int refs, int skip) { return j < refs && j != skip; }
  static __device__ __forceinline__ Entry entry(float d, int j) { return nn_key(d, j); }
  static __device__ __forceinline__ void put(float* w, int p, Entry e) {
    reinterpret_cast<unsigned*>(w)[2 * p] = (unsigned)e;
    reinterpret_cast<unsigned*>(w)[2 * p + 1] = (unsigned)(e >> 32);
  }
  static __device__ __forceinline__ Entry get(const float* w, int p) {
    return ((nnkey)reinterpret_cast<const unsigned*>(w)[2 * p + 1] << 32) | reinterpret_cast<const unsigned*>(w)[2 * p];
  }
  static __device__ __forceinline__ void store(Entry* __restrict__ o, const Entry (&l)[LIST]) {
#pragma unroll
    for (int p = 0; p < LIST; ++p) o[p] = l[p];
  }
};
static_assert(TM * LDT <= STAGE && TM * ValueList::WORDS <= STAGE && TM * KeyList::WORDS <= STAGE, "the epilogues reuse the staging buffers");

// The queries are the tile's ROWS (workgroup blockIdx.x takes 128 of them); the reference bank is walked as column tiles.  After each column tile
// the d2 tile goes to LDS (the accumulator layout spreads a row over lanes and registers); thread (row, half) merges 64 of the row's 128 columns
// into its own list, the two halves meet at the end.  part: [S][queries][LIST].  skip: the reference index left out of row a0 + row, or -1.
template <int V, class L>
__device__ __forceinline__ void list_partial(const float* __restrict__ qry, const float* __restrict__ nqry, int queries, const float* __restrict__ ref,
                                             const float* __restrict__ nref, int refs, const float* __restrict__ pivot,
                                             typename L::Entry* __restrict__ part, int D, int S, bool skip_self) {
  typedef typename L::Entry Entry;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  const int t = threadIdx.x, row = t & (TM - 1), half = t >> 7;
  const int a0 = blockIdx.x * TM, s = blockIdx.y;
  const int col_tiles = (refs + TM - 1) / TM;
  const int cb = (int)((long)s * col_tiles / S), ce = (int)((long)(s + 1) * col_tiles / S);
  float* na = smem + STAGE;
  if (t < TM) na[t] = a0 + t < queries ? nqry[a0 + t] : 0.f;
  Entry l[LIST];
#pragma unroll
  for (int p = 0; p < LIST; ++p) l[p] = L::empty();
  const int skip = skip_self ? a0 + row : -1;
  for (int ct = cb; ct < ce; ++ct) {
    const int b0 = ct * TM;
    f32x16 acc[2][2];
    tile_dot<V>(BankRows{qry, queries, a0}, BankRows{ref, refs, b0}, D, pivot, smem, acc);
    float nb[2];
    column_norms(nref, refs, b0, nb);
    for_each_acc(acc, [&](int il, int jl, int n, float dot) {
      smem[il * LDT + jl] = L::staged(a0 + il, b0 + jl, refs, d2_value(na[il], nb[n], dot));
    });
    __syncthreads();
    const float* mine = smem + row * LDT + half * 64;
    const int j0 = b0 + half * 64;
    for (int c = 0; c < 64; ++c)
      if (L::takes(j0 + c, refs, skip)) list_insert(l, L::entry(mine[c], j0 + c));
  }
  __syncthreads();
  float* hand = smem + row * L::WORDS;
  if (half == 1) {
#pragma unroll
    for (int p = 0; p < LIST; ++p) L::put(hand, p, l[p]);
  }
  __syncthreads();
  if (half == 0) {
#pragma unroll
    for (int p = 0; p < LIST; ++p) list_insert(l, L::get(hand, p));
    if (a0 + row < queries) L::store(part + ((long)s * queries + a0 + row) * LIST, l);
  }
}

// the k-NN radii: every row's 16 smallest d2 inside its own bank
template <int V>
__global__ __launch_bounds__(256, 2) void knn_partial_kernel(const float* __restrict__ x, const float* __restrict__ nx, const float* __restrict__ pivot,
                                                          float* __restrict__ part, int N, int D, int S) {
  list_partial<V, ValueList>(x, nx, N, x, nx, N, pivot, part, D, S, false);
}

// the neighbour search: the k <= 16 nearest of the N reference rows of every one of the M query rows, values AND indices, across two banks
template <int V>
__global__ __launch_bounds__(256, 2) void nn_partial_kernel(const float* __restrict__ qry, const float* __restrict__ nqry, const float* __restrict__ ref,
                                                         const float* __restrict__ nref, const float* __restrict__ pivot, nnkey* __restrict__ part, int N,
                                                         int M, int D, int S, int exclude_self) {
  list_partial<V, KeyList>(qry, nqry, M, ref, nref, N, pivot, part, D, S, exclude_self != 0);
}

// row i's S partial lists merged in ascending split order into l
template <class E>
__device__ __forceinline__ void merge_partials(const E* __restrict__ part, int i, int rows, int S, E (&l)[LIST]) {
  const E* q = part + (long)i * LIST;
#pragma unroll
  for (int p = 0; p < LIST; ++p) l[p] = q[p];
  for (int s = 1; s < S; ++s) {
    q = part + ((long)s * rows + i) * LIST;
    for (int p = 0; p < LIST; ++p) list_insert(l, q[p]);
  }
}

// r2[i] = the (knn + 1)-th smallest of row i, one thread per row
__global__ __launch_bounds__(256) void knn_finish_kernel(const float* __restrict__ part, float* __restrict__ r2, int N, int S, int knn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float l[LIST];
  merge_partials(part, i, N, S, l);
  float v = l[0];
#pragma unroll
  for (int p = 1; p < LIST; ++p) v = p == knn ? l[p] : v;
  r2[i] = v;
}

// d2[j][0 .. k) and index[j][0 .. k) of query j, one thread per query row
__global__ __launch_bounds__(256) void nn_finish_kernel(const nnkey* __restrict__ part, float* __restrict__ d2, int* __restrict__ index, int M, int S,
                                                        int k) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  nnkey l[LIST];
  merge_partials(part, i, M, S, l);
#pragma unroll
  for (int p = 0; p < LIST; ++p)
    if (p < k) {
      d2[(long)i * k + p] = __uint_as_float((unsigned)(l[p] >> 32));
      index[(long)i * k + p] = (int)(unsigned)l[p];
    }
}

// ---- epilogue 3: which reference rows' balls is query j inside?  [d2(R_i, Q_j) < r2_i], strict, over the reference tiles of split blockIdx.y: ANY of
// them as a flag (Count false), or their NUMBER (Count true).  The queries are the tile's COLUMNS: a lane owns two of them for the whole launch
// and ORs / counts over its registers, tile after tile; the four lanes that own a column (2 waves x 2 halves) meet in LDS -- a plain store of 1
// (several lanes may store the same 1), or an LDS integer add (integer sums: every order gives the same bits).
template <int V, bool Count>
__device__ __forceinline__ void manifold_partial(const float* __restrict__ ref, const float* __restrict__ nref, const float* __restrict__ r2,
                                                 const float* __restrict__ qry, const float* __restrict__ nqry, const float* __restrict__ pivot,
                                                 std::conditional_t<Count, int, uint8_t>* __restrict__ part, int NR, int M, int D, int S) {
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  const int t = threadIdx.x;
  const int b0 = blockIdx.x * TM, s = blockIdx.y;
  const int row_tiles = (NR + TM - 1) / TM;
  const int rb = (int)((long)s * row_tiles / S), re = (int)((long)(s + 1) * row_tiles / S);
  float* na = smem + STAGE;
  float* rad = na + TM;
  float nb[2];
  column_norms(nqry, M, b0, nb);
  std::conditional_t<Count, int, bool> in[2] = {};
  for (int rt = rb; rt < re; ++rt) {
    const int a0 = rt * TM;
    if (t < TM) {
      const bool row_in = a0 + t < NR;
      na[t] = row_in ? nref[a0 + t] : 0.f;
      rad[t] = row_in ? r2[a0 + t] : -1.f;     // d2 >= 0: a row past the end holds nobody
    }
    f32x16 acc[2][2];
    tile_dot<V>(BankRows{ref, NR, a0}, BankRows{qry, M, b0}, D, pivot, smem, acc);
    for_each_acc(acc, [&](int il, int, int n, float dot) {
      const bool inside = d2_value(na[il], nb[n], dot) < rad[il];
      if constexpr (Count) in[n] += inside ? 1 : 0;
      else in[n] = in[n] || inside;
    });
    __syncthreads();                       // na / rad are rewritten by the next tile
  }
  int* cols = reinterpret_cast<int*>(smem);
  if (t < TM) cols[t] = 0;
  __syncthreads();
  const int lane = t & 63, wc = (t >> 6) & 1;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    int* col = &cols[wc * 64 + n * 32 + (lane & 31)];
    if constexpr (Count) atomicAdd(col, in[n]);
    else if (in[n]) *col = 1;
  }
  __syncthreads();
  if (t < TM && b0 + t < M) part[(long)s * M + b0 + t] = cols[t];
}

template <int V>
__global__ __launch_bounds__(256, 2) void manifold_partial_kernel(const float* __restrict__ ref, const float* __restrict__ nref, const float* __restrict__ r2,
                                                               const float* __restrict__ qry, const float* __restrict__ nqry,
                                                               const float* __restrict__ pivot, uint8_t* __restrict__ part, int NR, int M, int D, int S) {
  manifold_partial<V, false>(ref, nref, r2, qry, nqry, pivot, part, NR, M, D, S);
}

template <int V>
__global__ __launch_bounds__(256, 2) void manifold_count_partial_kernel(const float* __restrict__ ref, const float* __restrict__ nref,
                                                                     const float* __restrict__ r2, const float* __restrict__ qry,
                                                                     const float* __restrict__ nqry, const float* __restrict__ pivot,
                                                                     int* __restrict__ part, int NR, int M, int D, int S) {
  manifold_partial<V, true>(ref, nref, r2, qry, nqry, pivot, part, NR, M, D, S);
}

// the sum of the 1024 threads' c by a fixed tree, as thread 0 sees it.  ONE workgroup of 1024.
template <class T>
__device__ __forceinline__ T tree_sum_1024(T* red, T c) {
  red[threadIdx.x] = c;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// hit[j] = the OR of the S partial flags in ascending split order; count = their number
__global__ __launch_bounds__(1024) void manifold_finish_kernel(const uint8_t* __restrict__ part, uint8_t* __restrict__ hit, int* __restrict__ count, int M,
                                                               int S) {
  __shared__ int red[1024];
  int c = 0;
  for (int j = threadIdx.x; j < M; j += 1024) {
    uint8_t f = 0;
    for (int s = 0; s < S; ++s) f |= part[(long)s * M + j];
    f = f ? 1 : 0;
    if (hit) hit[j] = f;
    c += f;
  }
  c = tree_sum_1024(red, c);
  if (threadIdx.x == 0 && count) *count = c;
}

// count[j] = the sum of the S partial counts; total = the sum of count[] as int64
__global__ __launch_bounds__(1024) void manifold_count_finish_kernel(const int* __restrict__ part, int* __restrict__ count, long long* __restrict__ total,
                                                                     int M, int S) {
  __shared__ long long red[1024];
  long long c = 0;
  for (int j = threadIdx.x; j < M; j += 1024) {
    int f = 0;
    for (int s = 0; s < S; ++s) f += part[(long)s * M + j];
    if (count) count[j] = f;
    c += f;
  }
  c = tree_sum_1024(red, c);
  if (threadIdx.x == 0 && total) *total = c;
}

// The fp64 sum over k of fl32(x_k - y_k)^2, in every lane of the wave: lane l takes k = l, l + 64, ... ascending, then a fixed shuffle tree.
// Element loads, so the result does not depend on the rows' alignment or place.
__device__ __forceinline__ double wave_sqsum(const float* __restrict__ x, const float* __restrict__ y, int D) {
  double s = 0.0;
  for (int k = threadIdx.x & 63; k < D; k += 64) {
    const float v = x[k] - y[k];
    s += (double)v * (double)v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// n(x) of every row: xt = fl32(x - c), the sum of xt^2 by wave_sqsum, rounded to fp32.  Four rows per workgroup, one wave each.
__global__ __launch_bounds__(256) void norms_kernel(const float* __restrict__ x, const float* __restrict__ pivot, float* __restrict__ out, int N, int D) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const double s = wave_sqsum(x + row * D, pivot, D);
  if ((threadIdx.x & 63) == 0) out[row] = (float)s;
}

// The exact distance of listed pairs: out[j][p] = fl32(wave_sqsum of q_j and r_i), i = index[j][p].  No pivot: a difference does not move under a
// shift.  One wave per pair.  The index is clamped into the bank BEFORE the load (a -1 never reaches memory); a pair whose index is outside the
// bank is stored as +inf.  Equal rows give exactly 0.
__global__ __launch_bounds__(256) void pair_sqdist_kernel(const float* __restrict__ qry, const float* __restrict__ ref, const int* __restrict__ index,
                                                          float* __restrict__ out, long pairs, int N, int D, int k) {
  const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= pairs) return;
  const int i = index[pair];
  const double s = wave_sqsum(qry + (pair / k) * D, ref + (long)min(max(i, 0), N - 1) * D, D);
  if ((threadIdx.x & 63) == 0) out[pair] = (unsigned)i < (unsigned)N ? (float)s : INFINITY;
}

// c[k] = the mean of column k in fp64, rounded to fp32.  A workgroup takes 32 columns; thread (column, phase p of 8) adds rows p, p + 8, ... in
// ascending order, the eight phases are added in ascending order.
__global__ __launch_bounds__(256) void colmean_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int D) {
  __shared__ double red[8][32];
  const int col = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const int k = blockIdx.x * 32 + col;
  double s = 0.0;
  if (k < D)
    for (long i = ph; i < N; i += 8) s += (double)x[i * D + k];
  red[ph][col] = s;
  __syncthreads();
  if (ph == 0 && k < D) {
    double a = red[0][col];
#pragma unroll
    for (int p = 1; p < 8; ++p) a += red[p][col];
    out[k] = (float)(a / (double)N);
  }
}

// tile `id` of the upper triangle of T x T tiles, rows ascending and ct >= rt ascending inside a row: row rt starts at rt T - rt (rt - 1) / 2
__device__ __forceinline__ void triangle_tile(long id, int T, int& rt, int& ct) {
  const double b = 2.0 * T + 1.0;
  long r = (long)((b - sqrt(b * b - 8.0 * (double)id)) * 0.5);
  r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
  while (r > 0 && r * T - r * (r - 1) / 2 > id) --r;
  while (r + 1 < T && (r + 1) * T - (r + 1) * r / 2 <= id) ++r;
  rt = (int)r;
  ct = (int)(r + id - (r * T - r * (r - 1) / 2));
}

// ---- epilogue 6: the SUM of k over one tile of one subset pair.  grid (the tiles of a subset pair, S subsets); subset s takes rows ia[s][0 .. sa) of
// bank A and ib[s][0 .. sb) of bank B (null: the identity).  Every lane adds its 64 elements in fp64 in for_each_acc's order, the 256 lanes meet in
// LDS by a fixed tree, one fp64 per tile goes to part[s][tile].  same (A is B, ia is ib): only the tiles with ct >= rt exist, an off-diagonal tile
// is stored twice over (exact in fp64), and with same == 1 a diagonal tile leaves p == q out, by position.  No atomics; the order is fixed in
// subset-local coordinates, so a gathered subset gives the bits of the same call on its materialised rows.
template <int V>
__global__ __launch_bounds__(256, 2) void ksum_partial_kernel(const float* __restrict__ a, const float* __restrict__ na, const int* __restrict__ ia,
                                                           const float* __restrict__ b, const float* __restrict__ nb, const int* __restrict__ ib,
                                                           const float* __restrict__ pivot, double* __restrict__ part, int N, int M, int D, int sa, int sb,
                                                           int col_tiles, int tiles, int same, KernelParams kp) {
  __shared__ __attribute__((aligned(16))) float smem[SMEM];
  const int t = threadIdx.x, s = blockIdx.y;
  int rt, ct;
  if (same) {
    triangle_tile(blockIdx.x, col_tiles, rt, ct);
  } else {
    rt = blockIdx.x / col_tiles;
    ct = blockIdx.x - rt * col_tiles;
  }
  const int a0 = rt * TM, b0 = ct * TM;
  const int* la = ia ? ia + (long)s * sa : nullptr;
  const int* lb = ib ? ib + (long)s * sb : nullptr;
  float* nas = smem + STAGE;
  if (t < TM) nas[t] = (na && a0 + t < sa) ? na[gather_index(la, a0 + t, sa, N)] : 0.f;
  float nbs[2];
  {
    const int lane = t & 63, wc = (t >> 6) & 1;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c = b0 + wc * 64 + n * 32 + (lane & 31);
      nbs[n] = (nb && c < sb) ? nb[gather_index(lb, c, sb, M)] : 0.f;
    }
  }
  f32x16 acc[2][2];
  tile_dot<V>(gather_rows(a, N, la, sa, a0, D, t), gather_rows(b, M, lb, sb, b0, D, t), D, pivot, smem, acc);
  const bool skip_diag = same == 1 && rt == ct;
  double sum = 0.0;
  for_each_acc(acc, [&](int il, int jl, int n, float dot) {
    const bool in = a0 + il < sa && b0 + jl < sb && !(skip_diag && il == jl);
    sum += in ? (double)kernel_value(kp, nas[il], nbs[n], dot) : 0.0;
  });
  double* red = reinterpret_cast<double*>(smem);      // (tile_dot left with a barrier: the staging buffers are free)
  red[t] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) part[(long)s * tiles + blockIdx.x] = (same && rt != ct) ? 2.0 * red[0] : red[0];
}

// out[s] = the sum of subset s's tile sums: thread t of the subset's workgroup adds the t-th run of ceil(tiles / 256) consecutive tiles in ascending
// order, thread 0 then adds the 256 runs in ascending order -- ascending tile order throughout, the same bits on every launch
__global__ __launch_bounds__(256) void ksum_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int tiles) {
  __shared__ double red[256];
  const int t = threadIdx.x, run = (tiles + 255) / 256;
  const double* p = part + (long)blockIdx.x * tiles;
  double s = 0.0;
  const long lo = (long)t * run, hi = min(lo + run, (long)tiles);
  for (long i = lo; i < hi; ++i) s += p[i];
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    double a = red[0];
    for (int i = 1; i < 256; ++i) a += red[i];
    out[blockIdx.x] = a;
  }
}

// the rules every descriptor of this unit shares, on the host, before any launch: the banks' sizes ...
int bank_rules(const char* what, int N, int M, int D) {
  MF_REQUIRE(N >= 1 && N < (1 << 24) && M >= 1 && M < (1 << 24), MF_EINVAL, "%s: N=%d M=%d (1 .. 2^24 - 1)", what, N, M);
  MF_REQUIRE(D >= 1 && D <= 65536, MF_EINVAL, "%s: D=%d (1 .. 65536)", what, D);
  return MF_OK;
}

// ... and, of an MfFidelityDesc, the splits and the same_bank flag
int split_rules(const MfFidelityDesc* d, const char* what) {
  MF_REQUIRE(d->splits >= 1 && d->splits <= MF_FIDELITY_MAX_SPLITS, MF_EINVAL, "%s: splits=%d (1 .. %d)", what, d->splits, MF_FIDELITY_MAX_SPLITS);
  MF_REQUIRE((d->same_bank & ~1) == 0, MF_EINVAL, "%s: same_bank is 0 or 1", what);
  MF_REQUIRE(!d->same_bank || d->M == d->N, MF_EINVAL, "%s: same_bank with N=%d M=%d", what, d->N, d->M);
  return MF_OK;
}

// the rules of precision / recall (mf_feat_sqdist_f32, mf_knn_*, mf_manifold_partial / finish)
int fidelity_rules(const MfFidelityDesc* d, const char* what) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  if (const int rc = bank_rules(what, d->N, d->M, d->D)) return rc;
  MF_REQUIRE(d->knn >= 1 && d->knn <= MF_FIDELITY_LIST - 1, MF_EINVAL, "%s: knn=%d (1 .. %d)", what, d->knn, MF_FIDELITY_LIST - 1);
  MF_REQUIRE(d->knn < d->N, MF_EINVAL, "%s: knn=%d needs more than %d rows", what, d->knn, d->N);
  return split_rules(d, what);
}

// the rules of the neighbour search and the counting launches (mf_nn_*, mf_pair_sqdist_f32, mf_manifold_count_*): knn is k, 1 .. 16, and may
// equal the reference rows (one less with same_bank, where a row is not its own neighbour)
int nn_rules(const MfFidelityDesc* d, const char* what) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  if (const int rc = bank_rules(what, d->N, d->M, d->D)) return rc;
  MF_REQUIRE(d->knn >= 1 && d->knn <= MF_FIDELITY_LIST, MF_EINVAL, "%s: k=%d (1 .. %d)", what, d->knn, MF_FIDELITY_LIST);
  if (const int rc = split_rules(d, what)) return rc;
  MF_REQUIRE(d->knn <= d->N - d->same_bank, MF_EINVAL, "%s: k=%d of %d reference rows%s", what, d->knn, d->N, d->same_bank ? " (the row itself left out)" : "");
  return MF_OK;
}

inline size_t nn_bytes(const MfFidelityDesc* d) { return (size_t)d->splits * d->M * LIST * sizeof(nnkey); }
inline size_t count_bytes(const MfFidelityDesc* d) { return ((size_t)d->splits * d->M * sizeof(int) + 15) & ~(size_t)15; }

inline size_t knn_bytes(const MfFidelityDesc* d) { return (size_t)d->splits * d->N * LIST * sizeof(float); }
inline size_t manifold_bytes(const MfFidelityDesc* d) { return ((size_t)d->splits * d->M + 15) & ~(size_t)15; }

// f(V) with V = 4 as a constant where every row of every bank can be loaded sixteen bytes at a time, V = 1 otherwise: the caller launches kernel<V>
template <class F>
inline void with_load_width(int D, std::initializer_list<const void*> ptrs, F f) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  if (D % 4 == 0 && (bits & 15) == 0)
    f(std::integral_constant<int, 4>{});
  else
    f(std::integral_constant<int, 1>{});
}

// the rules of the kernel sums and the kernel matrix (mf_ksum_*, mf_feat_kernel_f32)
int ksum_rules(const MfKernelSumDesc* d, const char* what) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  if (const int rc = bank_rules(what, d->N, d->M, d->D)) return rc;
  MF_REQUIRE(d->S >= 1 && d->S <= 65535, MF_EINVAL, "%s: S=%d (1 .. 65535)", what, d->S);
  MF_REQUIRE(d->sa >= 1 && d->sa <= d->N && d->sb >= 1 && d->sb <= d->M, MF_EINVAL, "%s: sa=%d sb=%d (1 .. N=%d, 1 .. M=%d)", what, d->sa, d->sb, d->N,
             d->M);
  MF_REQUIRE(d->kernel == MF_KERNEL_POLY || d->kernel == MF_KERNEL_RBF, MF_EINVAL, "%s: kernel=%d (0 poly, 1 rbf)", what, d->kernel);
  MF_REQUIRE(d->kernel != MF_KERNEL_POLY || (d->degree >= 1 && d->degree <= 4), MF_EINVAL, "%s: degree=%d (1 .. 4)", what, d->degree);
  MF_REQUIRE(std::isfinite(d->gamma) && d->gamma > 0.f, MF_EINVAL, "%s: gamma=%g (finite, positive)", what, (double)d->gamma);
  MF_REQUIRE(std::isfinite(d->coef0), MF_EINVAL, "%s: coef0=%g (finite)", what, (double)d->coef0);
  MF_REQUIRE(d->same_bank >= 0 && d->same_bank <= 2, MF_EINVAL, "%s: same_bank is 0, 1 or 2", what);
  MF_REQUIRE(!d->same_bank || (d->M == d->N && d->sb == d->sa), MF_EINVAL, "%s: same_bank with N=%d M=%d sa=%d sb=%d", what, d->N, d->M, d->sa, d->sb);
  MF_REQUIRE(d->reserved == 0, MF_EINVAL, "%s: reserved is 0", what);
  return MF_OK;
}

// the tiles one subset pair visits: all of them, or the upper triangle with its diagonal
inline long ksum_tiles(const MfKernelSumDesc* d) {
  const long ta = cdiv(d->sa, TM), tb = cdiv(d->sb, TM);
  return d->same_bank ? ta * (ta + 1) / 2 : ta * tb;
}
inline size_t ksum_bytes(const MfKernelSumDesc* d) { return ((size_t)d->S * (size_t)ksum_tiles(d) * sizeof(double) + 15) & ~(size_t)15; }
inline KernelParams kernel_params(const MfKernelSumDesc* d) { return KernelParams{d->kernel, d->degree, d->gamma, d->coef0}; }

}  // namespace

extern "C" {

int mf_fidelity_ok(const MfFidelityDesc* desc) { return fidelity_rules(desc, "fidelity_ok") == MF_OK ? 1 : 0; }

size_t mf_fidelity_workspace_bytes(const MfFidelityDesc* desc) {
  if (fidelity_rules(desc, "fidelity_workspace_bytes") != MF_OK) return 0;
  const size_t a = knn_bytes(desc), b = manifold_bytes(desc);
  return a > b ? a : b;
}

int mf_feat_colmean_f32(const float* x, float* pivot, int N, int D, void* stream) {
  MF_REQUIRE(x && pivot && N >= 1 && N < (1 << 24) && D >= 1 && D <= 65536, MF_EINVAL, "feat_colmean: N=%d D=%d", N, D);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)N * D, 4.0 * N * D);
  MF_LAUNCH(colmean_kernel, dim3(cdiv(D, 32)), dim3(256), 0, s, x, pivot, N, D);
  return check_launch("feat_colmean");
}

int mf_feat_norms_f32(const float* x, const float* pivot, float* norms, int N, int D, void* stream) {
  MF_REQUIRE(x && pivot && norms && N >= 1 && N < (1 << 24) && D >= 1 && D <= 65536, MF_EINVAL, "feat_norms: N=%d D=%d", N, D);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 3.0 * N * D, 4.0 * N * D);
  MF_LAUNCH(norms_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, x, pivot, norms, N, D);
  return check_launch("feat_norms");
}

int mf_feat_sqdist_f32(const float* x, const float* nx, const float* y, const float* ny, const float* pivot, float* out, const MfFidelityDesc* desc,
                       void* stream) {
  const int rc = fidelity_rules(desc, "feat_sqdist");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(x && nx && y && ny && pivot && out, MF_EINVAL, "feat_sqdist: bad args");
  MF_REQUIRE(!desc->same_bank || (x == y && nx == ny), MF_EINVAL, "feat_sqdist: same_bank with two banks");
  const long row_tiles = cdiv(desc->N, TM), col_tiles = cdiv(desc->M, TM);
  MF_REQUIRE(row_tiles * col_tiles <= 0x7fffffffL, MF_EINVAL, "feat_sqdist: %ld x %ld tiles", row_tiles, col_tiles);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->M * desc->D, 4.0 * ((double)desc->N * desc->M + ((double)desc->N + desc->M) * desc->D));
  const dim3 grid((unsigned)(row_tiles * col_tiles));
  with_load_width(desc->D, {x, y, pivot}, [&](auto v) {
    MF_LAUNCH(sqdist_kernel<decltype(v)::value>, grid, dim3(256), 0, s, x, nx, y, ny, pivot, out, desc->N, desc->M, desc->D, (int)col_tiles,
              desc->same_bank);
  });
  return check_launch("feat_sqdist");
}

int mf_knn_partial_f32(const float* x, const float* nx, const float* pivot, void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc,
                       void* stream) {
  const int rc = fidelity_rules(desc, "knn_partial");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(x && nx && pivot && workspace, MF_EINVAL, "knn_partial: bad args");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "knn_partial: a 16-byte aligned workspace");
  MF_REQUIRE(workspace_bytes >= knn_bytes(desc), MF_EWORKSPACE, "knn_partial: workspace of %zu bytes, %zu needed", workspace_bytes, knn_bytes(desc));
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->N * desc->D, 4.0 * desc->N * desc->D);
  const dim3 grid(cdiv(desc->N, TM), desc->splits);
  with_load_width(desc->D, {x, pivot}, [&](auto v) {
    MF_LAUNCH(knn_partial_kernel<decltype(v)::value>, grid, dim3(256), 0, s, x, nx, pivot, (float*)workspace, desc->N, desc->D, desc->splits);
  });
  return check_launch("knn_partial");
}

int mf_knn_finish_f32(const void* workspace, float* radii_sq, const MfFidelityDesc* desc, void* stream) {
  const int rc = fidelity_rules(desc, "knn_finish");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && radii_sq, MF_EINVAL, "knn_finish: bad args");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, (double)knn_bytes(desc));
  MF_LAUNCH(knn_finish_kernel, dim3(cdiv(desc->N, 256)), dim3(256), 0, s, (const float*)workspace, radii_sq, desc->N, desc->splits, desc->knn);
  return check_launch("knn_finish");
}

int mf_manifold_partial_f32(const float* ref, const float* nref, const float* radii_sq, const float* query, const float* nquery, const float* pivot,
                            void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc, void* stream) {
  const int rc = fidelity_rules(desc, "manifold_partial");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(ref && nref && radii_sq && query && nquery && pivot && workspace, MF_EINVAL, "manifold_partial: bad args");
  MF_REQUIRE(workspace_bytes >= manifold_bytes(desc), MF_EWORKSPACE, "manifold_partial: workspace of %zu bytes, %zu needed", workspace_bytes,
             manifold_bytes(desc));
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->M * desc->D, 4.0 * ((double)desc->N + desc->M) * desc->D);
  const dim3 grid(cdiv(desc->M, TM), desc->splits);
  with_load_width(desc->D, {ref, query, pivot}, [&](auto v) {
    MF_LAUNCH(manifold_partial_kernel<decltype(v)::value>, grid, dim3(256), 0, s, ref, nref, radii_sq, query, nquery, pivot, (uint8_t*)workspace, desc->N,
              desc->M, desc->D, desc->splits);
  });
  return check_launch("manifold_partial");
}

int mf_manifold_finish_f32(const void* workspace, uint8_t* hit, int32_t* count, const MfFidelityDesc* desc, void* stream) {
  const int rc = fidelity_rules(desc, "manifold_finish");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && (hit || count), MF_EINVAL, "manifold_finish: bad args");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, (double)manifold_bytes(desc));
  MF_LAUNCH(manifold_finish_kernel, dim3(1), dim3(1024), 0, s, (const uint8_t*)workspace, hit, count, desc->M, desc->splits);
  return check_launch("manifold_finish");
}

int mf_nn_ok(const MfFidelityDesc* desc) { return nn_rules(desc, "nn_ok") == MF_OK ? 1 : 0; }

size_t mf_nn_workspace_bytes(const MfFidelityDesc* desc) {
  if (nn_rules(desc, "nn_workspace_bytes") != MF_OK) return 0;
  return nn_bytes(desc);
}

int mf_nn_partial_f32(const float* query, const float* nquery, const float* ref, const float* nref, const float* pivot, void* workspace,
                      size_t workspace_bytes, const MfFidelityDesc* desc, void* stream) {
  const int rc = nn_rules(desc, "nn_partial");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(query && nquery && ref && nref && pivot && workspace, MF_EINVAL, "nn_partial: bad args");
  MF_REQUIRE(!desc->same_bank || (query == ref && nquery == nref), MF_EINVAL, "nn_partial: same_bank with two banks");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "nn_partial: a 16-byte aligned workspace");
  MF_REQUIRE(workspace_bytes >= nn_bytes(desc), MF_EWORKSPACE, "nn_partial: workspace of %zu bytes, %zu needed", workspace_bytes, nn_bytes(desc));
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->M * desc->D, 4.0 * ((double)desc->N + desc->M) * desc->D);
  const dim3 grid(cdiv(desc->M, TM), desc->splits);
  with_load_width(desc->D, {query, ref, pivot}, [&](auto v) {
    MF_LAUNCH(nn_partial_kernel<decltype(v)::value>, grid, dim3(256), 0, s, query, nquery, ref, nref, pivot, (nnkey*)workspace, desc->N, desc->M, desc->D,
              desc->splits, desc->same_bank);
  });
  return check_launch("nn_partial");
}

int mf_nn_finish_f32(const void* workspace, float* d2, int32_t* index, const MfFidelityDesc* desc, void* stream) {
  const int rc = nn_rules(desc, "nn_finish");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && d2 && index, MF_EINVAL, "nn_finish: bad args");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "nn_finish: a 16-byte aligned workspace");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, (double)nn_bytes(desc));
  MF_LAUNCH(nn_finish_kernel, dim3(cdiv(desc->M, 256)), dim3(256), 0, s, (const nnkey*)workspace, d2, index, desc->M, desc->splits, desc->knn);
  return check_launch("nn_finish");
}

int mf_pair_sqdist_f32(const float* query, const float* ref, const int32_t* index, float* out, const MfFidelityDesc* desc, void* stream) {
  const int rc = nn_rules(desc, "pair_sqdist");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(query && ref && index && out, MF_EINVAL, "pair_sqdist: bad args");
  hipStream_t s = (hipStream_t)stream;
  const long pairs = (long)desc->M * desc->knn;
  ProfScope ps(MF_FAM_MISC, s, 3.0 * pairs * desc->D, 8.0 * pairs * desc->D);
  MF_LAUNCH(pair_sqdist_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, query, ref, index, out, pairs, desc->N, desc->D, desc->knn);
  return check_launch("pair_sqdist");
}

int mf_manifold_count_partial_f32(const float* ref, const float* nref, const float* radii_sq, const float* query, const float* nquery,
                                  const float* pivot, void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc, void* stream) {
  const int rc = nn_rules(desc, "manifold_count_partial");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(ref && nref && radii_sq && query && nquery && pivot && workspace, MF_EINVAL, "manifold_count_partial: bad args");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "manifold_count_partial: a 16-byte aligned workspace");
  MF_REQUIRE(workspace_bytes >= count_bytes(desc), MF_EWORKSPACE, "manifold_count_partial: workspace of %zu bytes, %zu needed", workspace_bytes,
             count_bytes(desc));
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->M * desc->D, 4.0 * ((double)desc->N + desc->M) * desc->D);
  const dim3 grid(cdiv(desc->M, TM), desc->splits);
  with_load_width(desc->D, {ref, query, pivot}, [&](auto v) {
    MF_LAUNCH(manifold_count_partial_kernel<decltype(v)::value>, grid, dim3(256), 0, s, ref, nref, radii_sq, query, nquery, pivot, (int*)workspace,
              desc->N, desc->M, desc->D, desc->splits);
  });
  return check_launch("manifold_count_partial");
}

int mf_manifold_count_finish_f32(const void* workspace, int32_t* count, int64_t* total, const MfFidelityDesc* desc, void* stream) {
  const int rc = nn_rules(desc, "manifold_count_finish");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && (count || total), MF_EINVAL, "manifold_count_finish: bad args");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, (double)count_bytes(desc));
  MF_LAUNCH(manifold_count_finish_kernel, dim3(1), dim3(1024), 0, s, (const int*)workspace, count, (long long*)total, desc->M, desc->splits);
  return check_launch("manifold_count_finish");
}

int mf_ksum_ok(const MfKernelSumDesc* desc) { return ksum_rules(desc, "ksum_ok") == MF_OK && ksum_tiles(desc) <= 0x7fffffffL ? 1 : 0; }

size_t mf_ksum_workspace_bytes(const MfKernelSumDesc* desc) {
  if (ksum_rules(desc, "ksum_workspace_bytes") != MF_OK) return 0;
  if (ksum_tiles(desc) > 0x7fffffffL) {
    set_error("ksum_workspace_bytes: %ld tiles per subset pair", ksum_tiles(desc));
    return 0;
  }
  return ksum_bytes(desc);
}

int mf_ksum_partial_f32(const float* a, const float* na, const int32_t* ia, const float* b, const float* nb, const int32_t* ib, const float* pivot,
                        void* workspace, size_t workspace_bytes, const MfKernelSumDesc* desc, void* stream) {
  const int rc = ksum_rules(desc, "ksum_partial");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(a && b && pivot && workspace, MF_EINVAL, "ksum_partial: bad args");
  MF_REQUIRE(desc->kernel != MF_KERNEL_RBF || (na && nb), MF_EINVAL, "ksum_partial: the rbf kernel needs the norms of both banks");
  MF_REQUIRE(!desc->same_bank || (a == b && na == nb && ia == ib), MF_EINVAL, "ksum_partial: same_bank with two banks or two index lists");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "ksum_partial: a 16-byte aligned workspace");
  const long tiles = ksum_tiles(desc);
  MF_REQUIRE(tiles <= 0x7fffffffL, MF_EINVAL, "ksum_partial: %ld tiles per subset pair", tiles);
  MF_REQUIRE(workspace_bytes >= ksum_bytes(desc), MF_EWORKSPACE, "ksum_partial: workspace of %zu bytes, %zu needed", workspace_bytes, ksum_bytes(desc));
  hipStream_t s = (hipStream_t)stream;
  const double pairs = (double)desc->S * desc->sa * desc->sb * (desc->same_bank ? 0.5 : 1.0);
  ProfScope ps(MF_FAM_MISC, s, 2.0 * pairs * desc->D, 4.0 * desc->S * ((double)desc->sa + desc->sb) * desc->D);
  const dim3 grid((unsigned)tiles, (unsigned)desc->S);
  const int col_tiles = cdiv(desc->sb, TM);
  with_load_width(desc->D, {a, b, pivot}, [&](auto v) {
    MF_LAUNCH(ksum_partial_kernel<decltype(v)::value>, grid, dim3(256), 0, s, a, na, ia, b, nb, ib, pivot, (double*)workspace, desc->N, desc->M, desc->D,
              desc->sa, desc->sb, col_tiles, (int)tiles, desc->same_bank, kernel_params(desc));
  });
  return check_launch("ksum_partial");
}

int mf_ksum_finish_f64(const void* workspace, double* out, const MfKernelSumDesc* desc, void* stream) {
  const int rc = ksum_rules(desc, "ksum_finish");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && out, MF_EINVAL, "ksum_finish: bad args");
  MF_REQUIRE(((uintptr_t)workspace & 15) == 0, MF_EINVAL, "ksum_finish: a 16-byte aligned workspace");
  const long tiles = ksum_tiles(desc);
  MF_REQUIRE(tiles <= 0x7fffffffL, MF_EINVAL, "ksum_finish: %ld tiles per subset pair", tiles);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, (double)ksum_bytes(desc));
  MF_LAUNCH(ksum_finish_kernel, dim3((unsigned)desc->S), dim3(256), 0, s, (const double*)workspace, out, (int)tiles);
  return check_launch("ksum_finish");
}

int mf_feat_kernel_f32(const float* x, const float* nx, const float* y, const float* ny, const float* pivot, float* out, const MfKernelSumDesc* desc,
                       void* stream) {
  const int rc = ksum_rules(desc, "feat_kernel");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(x && y && pivot && out, MF_EINVAL, "feat_kernel: bad args");
  MF_REQUIRE(desc->kernel != MF_KERNEL_RBF || (nx && ny), MF_EINVAL, "feat_kernel: the rbf kernel needs the norms of both banks");
  const long row_tiles = cdiv(desc->N, TM), col_tiles = cdiv(desc->M, TM);
  MF_REQUIRE(row_tiles * col_tiles <= 0x7fffffffL, MF_EINVAL, "feat_kernel: %ld x %ld tiles", row_tiles, col_tiles);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * desc->N * desc->M * desc->D, 4.0 * ((double)desc->N * desc->M + ((double)desc->N + desc->M) * desc->D));
  const dim3 grid((unsigned)(row_tiles * col_tiles));
  with_load_width(desc->D, {x, y, pivot}, [&](auto v) {
    MF_LAUNCH(kernel_matrix_kernel<decltype(v)::value>, grid, dim3(256), 0, s, x, nx, y, ny, pivot, out, desc->N, desc->M, desc->D, (int)col_tiles,
              kernel_params(desc));
  });
  return check_launch("feat_kernel");
}

}  // extern "C"
