// conv_f16x2_epilogue.inc -- the epilogue of the fp16-pair convolution kernels, included textually INSIDE their bodies (conv_f16x2.h:
// conv_f16x2_kernel; conv_f16x2_halo.h: conv_halo_kernel): in-launch split-K tree, scaling, staging through LDS, bias, NHWC stores, bound
// slots, GroupNorm partial records.  Expects in scope: p, smem, tid, lane, wave, wm, wn, fh, m0, n0, tile_m, tile_n, kz, last_src2, accm, accx,
// the constants BM, BN, WM, WN, NW, FM, FN, TM, TN, the macros MFC2_PIXEL_EXPS / MFC2_WAIT_LGKM0 / MFC2_WAIT_VM / MFC2_HZ_ON, and
// MFC2_EPILOGUE_LDS_BYTES = the LDS bytes that are dead once the main loop is over.
  // ---- epilogue.  D[cout][pixel]: lane holds pixel (lane & 31) and couts (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of each 32 x 32 block.
  // All DMA has landed (the last iterations wait vmcnt(0)); the stages are dead once every wave has left the loop.
  MFC2_WAIT_LGKM0();
  __builtin_amdgcn_s_barrier();
  MFC2_STAMP(4)
  if constexpr (MFC2_HZ_ON(0)) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  if (p.tree) {   // ---- split-K met inside the launch (see ConvP2)
    // the accumulators become the values of this K slice, (main + cross / 2048) x 2^(operand scales); `accx` is cleared so that the
    // epilogue below, which forms the same expression for the other launches, reproduces them (f_out = 1 there)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      MFC2_PIXEL_EXPS(i)
      const float f_out = exp2i(last_src2 ? e2_ : e1_) * exp2i(p.wexp);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accm[i][j][r] = (accm[i][j][r] + accx[i][j][r] * kLoInv) * f_out; accx[i][j][r] = 0.f; }
    }
    constexpr int SLOT = BM * BN;                       // floats per hand-off slot; inside a slot: [wave][i][j][q][lane][4]
    const int tile = tile_n * p.tiles_m + tile_m;
    float* region = p.handoff + (long)tile * (2L * (p.splitk - 1)) * SLOT;
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(region, 0, (unsigned)(2 * (p.splitk - 1)) * (unsigned)SLOT * 4u, 0x00020000);
    unsigned* cnt = p.sync + (long)tile * (p.splitk - 1);
    unsigned* flag = reinterpret_cast<unsigned*>(smem);   // (the pipeline stages are dead)
    const unsigned lane_off = (unsigned)((wave * TM * TN * 4) * 64 + lane) * 16u;
    int lbase = 0;
    for (int span = 1; span < p.splitk; span <<= 1) {
      if constexpr (MFC2_HZ_ON(4)) asm volatile("s_nop 15" ::: "memory");
      const int lv = __builtin_ctz(span);
      const int side = (kz >> lv) & 1, pair = kz >> (lv + 1);
      const unsigned mine = (unsigned)(2 * (lbase + pair) + side) * (unsigned)SLOT * 4u, theirs = (unsigned)(2 * (lbase + pair) + (side ^ 1)) * (unsigned)SLOT * 4u;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            u32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __float_as_uint(accm[i][j][4 * q + e]);
            __builtin_amdgcn_raw_buffer_store_b128(v, rh, lane_off + (unsigned)(((i * TN + j) * 4 + q) * 1024), mine, 0x10);   // sc1: agent scope, write-through
          }
      MFC2_WAIT_VM(0);
      if constexpr (MFC2_HZ_ON(4)) asm volatile("s_nop 15" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        // Publication.  The payload went out as 16-byte sc1 (write-through, agent scope) stores that every wave has waited for
        // (vmcnt(0) + barrier above), the partner reads it with sc1 loads behind the counter: the {sc1 stores, sc1 loads} hand-off of
        // MI355X_MICROARCH.md "Workgroup dispatch ... visibility".  tree == 2 adds the memory model's own fences around the counter
        // (release = buffer_wbl2 sc1 + vmcnt(0) before the bump, acquire = buffer_inv sc1 after the second arriver's bump; one lane,
        // then the barrier below) -- the form that does not lean on cache-policy bits; MF_CONV_TREE selects (conv_f16x2.hip).
        if (p.tree == 2) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          MFC2_WAIT_VM(0);   // (restated where the compiler cannot drop it: ROCm 7.2 elides the wait behind buffer_wbl2 after an explicit vmcnt(0))
        }
        const unsigned old = __hip_atomic_fetch_add(cnt + lbase + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old) __hip_atomic_store(cnt + lbase + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // second: nobody touches it again in this launch
        if (p.tree == 2 && old) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        *flag = old;
      }
      __syncthreads();
      const unsigned second = *flag;
      __syncthreads();   // (the flag word is rewritten at the next level)
      if (!second) return;            // the partner finishes this tile
      if constexpr (MFC2_HZ_ON(3)) {   // every load landed before the first add
        u32x4 pv[TM * TN * 4];
#pragma unroll
        for (int u = 0; u < TM * TN * 4; ++u) pv[u] = __builtin_amdgcn_raw_buffer_load_b128(rh, lane_off + (unsigned)(u * 1024), theirs, 0x10);
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 7" ::: "memory");
#if MFC2_HZ & 256
        if (p.dbg) {   // [1]: this workgroup's own values, [2]: what it loaded from its partner (layout of [0], the sum dumped behind the tree)
          const long plane = (long)p.tiles_m * p.tiles_n * NW * (TM * TN * 16 * 64);
          float* o = p.dbg + ((long)tile * NW + wave) * (TM * TN * 16 * 64) + lane;
#pragma unroll
          for (int u = 0; u < TM * TN * 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              __builtin_nontemporal_store(accm[u / (4 * TN)][(u / 4) % TN][4 * (u % 4) + e], o + plane + (u * 4 + e) * 64);
              __builtin_nontemporal_store(__uint_as_float(pv[u][e]), o + 2 * plane + (u * 4 + e) * 64);
            }
        }
#endif
#pragma unroll
        for (int u = 0; u < TM * TN * 4; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) accm[u / (4 * TN)][(u / 4) % TN][4 * (u % 4) + e] += __uint_as_float(pv[u][e]);
      } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rh, lane_off + (unsigned)(((i * TN + j) * 4 + q) * 1024), theirs, 0x10);   // sc1: past this XCD's L2
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if constexpr (MFC2_HZ_ON(5)) accm[i][j][4 * q + e] = hz_add(accm[i][j][4 * q + e], __uint_as_float(v[e]));
              else accm[i][j][4 * q + e] += __uint_as_float(v[e]);
            }
          }
      }
      lbase += p.splitk >> (lv + 1);
    }
#if MFC2_HZ & 256
    if (p.dbg) {
      float* o = p.dbg + ((long)tile * NW + wave) * (TM * TN * 16 * 64) + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) __builtin_nontemporal_store(accm[i][j][r], o + ((i * TN + j) * 16 + r) * 64);
    }
#endif
  }
  MFC2_STAMP(5)
  const bool last_slice = p.splitk == 1 || p.tree;   // this workgroup holds final values: bias, statistics, bounds
  constexpr int PITCH = FN * 4 + 16;                  // wave-private staging rows [32 pixels][FN couts] fp32 (+16 B: conflict-free b128 writes)
  char* stg = smem + wave * (32 * PITCH);
  static_assert(NW * 32 * PITCH <= MFC2_EPILOGUE_LDS_BYTES, "epilogue staging must fit in the pipeline stages");
  constexpr int LPR = FN / 8, RPP = 64 / LPR, NPASS = 32 / RPP;   // lanes per pixel row (8 couts each), rows per pass, passes per sub-tile
  const int rr = lane / LPR, c8 = lane % LPR;
  const int col0 = n0 + wn * FN + c8 * 8;
  float* out = p.y + (last_slice ? 0L : (long)kz * p.slab);
#if MFC2_OUT_STORE == 2
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, (unsigned)((long)p.M * p.Cout * 4), 0x00020000);
#endif
#if MFC2_EXPS_EARLY
  // the bias was fetched in the ramp (MFC2_EXPS_EARLY == 2: at the entry, waited for in front of the first DMA -- nothing is pending here; == 1:
  // behind the prologue's DMA).  It must be KNOWN to have arrived before the store passes below: they sit under
  // per-row `if (m < M)` branches, and with a load still pending on some path the compiler re-waits vmcnt(0) in every pass -- which on this
  // target also waits for the previous pass's output STORES (they count in vmcnt): eight serialised store round trips per workgroup,
  // 2.9 us of a 57 us launch (scripts/conv_timeline.py).  The empty asm is a use in straight-line code: one wait, here.
  f32x4 b0 = eb0, b1 = eb1;
  asm volatile("" : "+v"(b0), "+v"(b1));
#else
  f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
  if (last_slice && p.bias) {
    b0 = *reinterpret_cast<const f32x4*>(p.bias + col0);
    b1 = *reinterpret_cast<const f32x4*>(p.bias + col0 + 4);
  }
#endif
  float s1 = 0.f, s2 = 0.f, vmax = 0.f;
  const bool fz = p.fz.on != 0;    // GroupNorm + Swish + residual + embedding applied in THIS launch (conv_f16x2.h: FuseP): the rows stay in registers
  f32x4 yk0[TM][NPASS], yk1[TM][NPASS];
#pragma unroll
  for (int i = 0; i < TM; ++i) {   // one 32-pixel sub-tile at a time through the wave's staging region (LDS operations of a wave stay in order)
    MFC2_PIXEL_EXPS(i)
    const float f_out = p.tree ? 1.f : exp2i(last_src2 ? e2_ : e1_) * exp2i(p.wexp);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (MFC2_HZ_ON(6)) v[e] = hz_mul(hz_add(accm[i][j][4 * q + e], hz_mul(accx[i][j][4 * q + e], kLoInv)), f_out);
          else v[e] = (accm[i][j][4 * q + e] + accx[i][j][4 * q + e] * kLoInv) * f_out;
        }
        *reinterpret_cast<f32x4*>(stg + (lane & 31) * PITCH + (j * 32 + 8 * q + 4 * fh) * 4) = v;
        if constexpr (MFC2_HZ_ON(7)) asm volatile("s_nop 0" ::: "memory");
        if constexpr (MFC2_HZ_ON(1)) asm volatile("s_nop %1" : "+v"(v) : "n"(MFC2_HZ_PAD) : "memory");   // the data registers stay untouched for PAD + 1 states
      }
    f32x4 rv0[NPASS], rv1[NPASS];   // every read of the sub-tile first (one LDS round trip instead of NPASS), then the passes
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      rv0[ps] = *reinterpret_cast<const f32x4*>(stg + (ps * RPP + rr) * PITCH + c8 * 32);
      rv1[ps] = *reinterpret_cast<const f32x4*>(stg + (ps * RPP + rr) * PITCH + c8 * 32 + 16);
    }
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      const int row = ps * RPP + rr;
      f32x4 v0 = rv0[ps], v1 = rv1[ps];
      if constexpr (MFC2_HZ_ON(2)) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 3" : "+v"(v0), "+v"(v1)::"memory");
      v0 += b0;
      v1 += b1;
      const int m = m0 + wm * FM + i * 32 + row;
      yk0[i][ps] = v0;
      yk1[i][ps] = v1;
      if (fz) {
        if (m < p.M) {   // the statistics, in the order of the branch below (the records of the two forms are bit-identical)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s1 += v0[e] + v1[e];
            s2 = fmaf(v0[e], v0[e], s2);
            s2 = fmaf(v1[e], v1[e], s2);
          }
        }
      } else if (m < p.M) {
        long orow = m;
        if (p.subpix) {  // row m = (n, phase, y, x) -> output pixel (n, 2y + a, 2x + b)
          const int n = m / p.HWout, rem = m - n * p.HWout;
          const int ph = rem / p.hw_src, r2 = rem - ph * p.hw_src;
          const int y = r2 / p.Win, x = r2 - y * p.Win;
          orow = ((long)n * p.Hout + 2 * y + (ph >> 1)) * p.Wout + 2 * x + (ph & 1);
        }
#if MFC2_OUT_STORE == 1   /* experiment: non-temporal output stores (the end-of-kernel write-back finds nothing dirty) */
        __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(out + orow * p.Cout + col0));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(out + orow * p.Cout + col0 + 4));
#elif MFC2_OUT_STORE == 2   /* experiment (round 4): write-through (sc1) output stores -- nothing stays dirty in the XCD's L2, so the kernel boundary
                               behind this launch has no write-back to wait for (MI355X_MICROARCH.md, "boundary": + dirty bytes / 6 TB/s) */
        {
          const unsigned ob_ = (unsigned)((orow * p.Cout + col0) * 4);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v0), rs_out, ob_, 0, 0x10);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v1), rs_out, ob_ + 16u, 0, 0x10);
        }
#else
        if (p.out_nt) {
          __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(out + orow * p.Cout + col0));
          __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(out + orow * p.Cout + col0 + 4));
        } else {
          *reinterpret_cast<f32x4*>(out + orow * p.Cout + col0) = v0;
          *reinterpret_cast<f32x4*>(out + orow * p.Cout + col0 + 4) = v1;
        }
#endif
        if (p.out_bound) {
#pragma unroll
          for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
        }
        if (p.y_pairs) {   // the fp16-pair form under the derived bound of the row's sample (ConvP2::y_pairs)
          const int nrow = m / p.HWout;
          const float yb = p.bound1[nrow] * p.wl1_1 + (p.C2 > 0 ? p.bound2[nrow] * p.wl1_2 : 0.f) + p.bmax;
          const float ysc = exp2i(-scale_exp_of(yb));
          sf_u32x4 hi, lo;
          split8_f16<false>(v0 * ysc, v1 * ysc, hi, lo);
          sf_u32x4* op = reinterpret_cast<sf_u32x4*>(reinterpret_cast<char*>(p.y_pairs) + ((orow * p.Cout + col0) >> 3) * 32);
          op[0] = hi;
          op[1] = lo;
          if (m - nrow * p.HWout == 0 && col0 == 0) p.y_pair_bound[nrow] = yb;   // (one lane per sample: its first row, first channel octet)
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s1 += v0[e] + v1[e];
          s2 = fmaf(v0[e], v0[e], s2);
          s2 = fmaf(v1[e], v1[e], s2);
        }
      }
    }
  }
  MFC2_STAMP(6)
  // A tile lies inside one sample (HWout % BM == 0), or -- small images -- holds BM / HWout whole samples, each a whole number of wave rows
  // (HWout % FM == 0): the host guarantees one of the two whenever it asks for bounds or statistics.
  const int wm_per_sample = p.HWout >= BM ? WM : p.HWout / FM;            // wave rows (wm) per sample inside this tile
  const int n_first = m0 / p.HWout;                                        // first sample of the tile
  if (p.out_bound) {   // slot (tile inside the sample, n-tile, wave inside the sample) of the wave's sample
    vmax = wave_max(vmax);
    const int n = n_first + wm / wm_per_sample;
    const int part = p.HWout >= BM ? (m0 - n_first * p.HWout) / BM : 0;
    const int wps = wm_per_sample * WN;                                    // waves per sample
    if (lane == 0 && n < p.N) p.out_bound[(long)n * p.bound_slots + (part * p.tiles_n + tile_n) * wps + (wm % wm_per_sample) * WN + wn] = vmax;
  }
  if (p.gn_partial) {  // host guarantees: this workgroup holds final values, BN % cpg == 0, cpg % 8 == 0
    // a lane holds the fp32 sums of its 8 couts over its rows; the RPP lanes of a wave with the same couts add up in fp64 by shuffles,
    // then ONE value pair per (wave, 8-cout slot) goes through LDS and the first threads add the few slots / wave rows of their group
    double d1 = (double)s1, d2 = (double)s2;
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
      d1 += __shfl_xor(d1, off, 64);
      d2 += __shfl_xor(d2, off, 64);
    }
    __builtin_amdgcn_s_barrier();   // every wave has finished with its staging region
    double* red = reinterpret_cast<double*>(smem);   // [NW waves][LPR slots][2]
    if (lane < LPR) {
      red[(wave * LPR + lane) * 2] = d1;
      red[(wave * LPR + lane) * 2 + 1] = d2;
    }
    MFC2_WAIT_LGKM0();
    __builtin_amdgcn_s_barrier();
    const int ngl = BN / p.gn_cpg, spt = WM / wm_per_sample;               // groups in the tile's channel range, samples per tile
    if (tid < ngl * spt) {
      const int gl = tid % ngl, si = tid / ngl;
      double s = 0, q = 0;
      const int slots = p.gn_cpg >> 3;
      for (int k = 0; k < slots; ++k) {
        const int slot8 = gl * slots + k;
        const int wn_ = slot8 / LPR, c8_ = slot8 - wn_ * LPR;
        for (int wm_ = si * wm_per_sample; wm_ < (si + 1) * wm_per_sample; ++wm_) {
          const double* d = red + ((wm_ * WN + wn_) * LPR + c8_) * 2;
          s += d[0];
          q += d[1];
        }
      }
      const int n = n_first + si;
      const int part = p.HWout >= BM ? (m0 - n_first * p.HWout) / BM : 0;
      if (n < p.N) {
        double* o = p.gn_partial + (((long)n * p.gn_parts + part) * p.gn_groups + (n0 / p.gn_cpg + gl)) * 2;
        if (fz) {   // read by the other workgroups of the sample inside this launch: 8-byte agent-scope stores (write-through), agent-scope loads there
          __hip_atomic_store(o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(o + 1, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          o[0] = s;
          o[1] = q;
        }
      }
    }
  }
  if (fz) {
    // ---- the fused GroupNorm-apply tail (conv_f16x2.h: FuseP).  Host guarantees: gn_partial set, every workgroup of the launch resident.
    // (1) publish: every record store of this workgroup has been acknowledged, then ONE arrival per sample of the tile
    MFC2_WAIT_VM(0);
    __syncthreads();
    const int spt = WM / wm_per_sample;                 // whole samples in this tile (1: the tile lies inside one sample)
    const int ngl_ = BN / p.gn_cpg;                     // groups in the tile's channel range
    const unsigned T_ = (unsigned)p.fz.tiles_per_sample;
    if (tid == 0) {
      for (int si = 0; si < spt; ++si) {
        const int n = n_first + si;
        if (n < p.N) __hip_atomic_fetch_add(p.fz.rv + 2 * n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    MFC2_STAMP(6)   // (fused launches: 6 = records published + arrival, 7 = the sample is complete, 3 = end of the tail)
    // (2) what does not depend on the other workgroups, while they arrive: bounds, channel constants, the residual rows
    const int si_w = wm / wm_per_sample;                // this wave's sample inside the tile
    const int n_w = min(n_first + si_w, p.N - 1);       // (a wave past the last sample stores nothing: its rows are >= M)
    float* fzs = reinterpret_cast<float*>(smem + 8192); // [si * 8 + wave] slot maxima, [64]: wait result, [128 + (si * ngl + gl) * 2] mean, rstd
    float rb = 0.f;
    if (p.fz.res_slots) {   // the residual's measured bound straight from the slots its convolution wrote (max: any order gives the same bits)
      for (int si = 0; si < spt; ++si) {
        const int n = min(n_first + si, p.N - 1);
        float mx = 0.f;
        for (int k = tid; k < p.fz.res_nslots; k += NW * 64) mx = fmaxf(mx, p.fz.res_slots[(long)n * p.fz.res_nslots + k]);
        mx = wave_max(mx);
        if (lane == 0) fzs[si * 8 + wave] = mx;
      }
      MFC2_WAIT_LGKM0();
      __syncthreads();
#pragma unroll
      for (int w8 = 0; w8 < NW; ++w8) rb = fmaxf(rb, fzs[si_w * 8 + w8]);
    } else if (p.fz.res_bound) {
      rb = p.fz.res_bound[n_w];
    }
    const float ob_ = p.fz.bconst + rb + (p.fz.emb_bound ? p.fz.emb_bound[n_w] : 0.f);      // (the order of mf_gn_apply_*: bconst + residual + embedding)
    const float osc = exp2i(-scale_exp_of(ob_));
    const float rsc = p.fz.res_pairs ? exp2i(scale_exp_of(p.fz.res_bound[n_w])) : 1.f;
    {
      const int part0 = p.HWout >= BM ? (m0 - n_first * p.HWout) / BM : 0;
      if (tile_n == 0 && part0 == 0 && wn == 0 && (wm % wm_per_sample) == 0 && lane == 0 && n_first + si_w < p.N) p.fz.out_bound[n_first + si_w] = ob_;
    }
    f32x4 ga0 = {1.f, 1.f, 1.f, 1.f}, ga1 = ga0, be0 = {0.f, 0.f, 0.f, 0.f}, be1 = be0, em0 = be0, em1 = be0;
    if (p.fz.gamma) {
      ga0 = *reinterpret_cast<const f32x4*>(p.fz.gamma + col0); ga1 = *reinterpret_cast<const f32x4*>(p.fz.gamma + col0 + 4);
      be0 = *reinterpret_cast<const f32x4*>(p.fz.beta + col0);  be1 = *reinterpret_cast<const f32x4*>(p.fz.beta + col0 + 4);
    }
    if (p.fz.emb) {
      const float* er = p.fz.emb + (long)n_w * p.fz.emb_stride + col0;
      em0 = *reinterpret_cast<const f32x4*>(er); em1 = *reinterpret_cast<const f32x4*>(er + 4);
    }
    f32x4 rk0[TM][NPASS], rk1[TM][NPASS];   // residual rows: fp32 values, or the raw [hi x 8 | lo' x 8] pieces of the pair form
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int m = m0 + wm * FM + i * 32 + ps * RPP + rr;
        rk0[i][ps] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk1[i][ps] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (m < p.M) {
          const long e = (long)m * p.Cout + col0;
          if (p.fz.res_pairs) {
            const f32x4* g = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.fz.res_pairs) + (e >> 3) * 32);
            rk0[i][ps] = g[0]; rk1[i][ps] = g[1];
          } else if (p.fz.res_f32) {
            rk0[i][ps] = *reinterpret_cast<const f32x4*>(p.fz.res_f32 + e); rk1[i][ps] = *reinterpret_cast<const f32x4*>(p.fz.res_f32 + e + 4);
          }
        }
      }
    // (3) wait for every sample of the tile (one lane polls; a bounded wait: see FuseP)
    if (tid == 0) {
      unsigned ok = 1u;
      for (int si = 0; si < spt; ++si) {
        const int n = n_first + si;
        if (n >= p.N) continue;
        const unsigned long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
        unsigned spins = 0;
        while (__hip_atomic_load(p.fz.rv + 2 * n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < T_) {
          __builtin_amdgcn_s_sleep(1);
          if ((++spins & 127u) == 0u) {
            if (__hip_atomic_load(p.fz.rv_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 0u; break; }
            if (__builtin_amdgcn_s_memrealtime() - t0 > 5000000ul) {
              __hip_atomic_store(p.fz.rv_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              ok = 0u;
              break;
            }
          }
        }
      }
      reinterpret_cast<unsigned*>(fzs)[64] = ok;
    }
    MFC2_WAIT_LGKM0();
    __syncthreads();
    MFC2_STAMP(7)
    // (4) mean / rstd of the tile's groups from the records of the WHOLE sample: the summation order of gn_apply_part_kernel (groupnorm.hip)
    // -- PPT = 256 / G interleaved sub-sums, added in order -- and its formula, so that the two forms agree bit for bit
    if (tid < ngl_ * spt) {
      const int gl = tid % ngl_, si = tid / ngl_;
      const int n = n_first + si;
      if (n < p.N) {
        const int G_ = p.gn_groups, PPT = 256 / G_, g = n0 / p.gn_cpg + gl;
        double S = 0, Q = 0;
        for (int kk = 0; kk < PPT; ++kk) {
          double a = 0, b = 0;
          for (int k = kk; k < p.gn_parts; k += PPT) {
            const double* r_ = p.gn_partial + (((long)n * p.gn_parts + k) * G_ + g) * 2;
            a += __hip_atomic_load(r_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b += __hip_atomic_load(r_ + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (kk == 0) { S = a; Q = b; } else { S += a; Q += b; }
        }
        const double mean = S / p.fz.count;
        double var = Q / p.fz.count - mean * mean;
        if (var < 0) var = 0;
        fzs[128 + (si * ngl_ + gl) * 2] = (float)mean;
        fzs[128 + (si * ngl_ + gl) * 2 + 1] = (float)(1.0 / sqrt(var + (double)p.fz.eps));
      }
    }
    MFC2_WAIT_LGKM0();
    __syncthreads();
    // (5) depart: the last workgroup of a sample to leave its wait zeroes the pair of counters (every other one has passed its poll)
    if (tid == 0) {
      for (int si = 0; si < spt; ++si) {
        const int n = n_first + si;
        if (n >= p.N) continue;
        const unsigned old = __hip_atomic_fetch_add(p.fz.rv + 2 * n + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == T_) {
          __hip_atomic_store(p.fz.rv + 2 * n, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(p.fz.rv + 2 * n + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // (6) normalise, Swish, residual, embedding -- the per-element arithmetic of gn_apply_part_kernel, same operations in the same order --
    // and out: fp16 pairs (32 contiguous bytes per lane: [hi x 8][lo' x 8]) and, where a consumer needs it, fp32
    const int glw = (wn * FN + c8 * 8) / p.gn_cpg;
    const float mean_ = fzs[128 + (si_w * ngl_ + glw) * 2], rstd_ = fzs[128 + (si_w * ngl_ + glw) * 2 + 1];
    const bool aff = p.fz.gamma != nullptr, act1 = p.fz.act == 1, resp = p.fz.res_pairs != nullptr, resf = !resp && p.fz.res_f32 != nullptr,
               hasemb = p.fz.emb != nullptr;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int m = m0 + wm * FM + i * 32 + ps * RPP + rr;
        if (m < p.M) {
          float ev[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { ev[e] = yk0[i][ps][e]; ev[4 + e] = yk1[i][ps][e]; }
          const float gv[8] = {ga0[0], ga0[1], ga0[2], ga0[3], ga1[0], ga1[1], ga1[2], ga1[3]};
          const float bv[8] = {be0[0], be0[1], be0[2], be0[3], be1[0], be1[1], be1[2], be1[3]};
          const float mv[8] = {em0[0], em0[1], em0[2], em0[3], em1[0], em1[1], em1[2], em1[3]};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float t = (ev[e] - mean_) * rstd_;
            if (aff) t = t * gv[e] + bv[e];
            if (act1) t = swish_apply(t);
            ev[e] = t;
          }
          if (resp) {   // [hi x 8] in rk0, [lo' x 8] in rk1: value = (hi + lo' / 2048) 2^s
            const u32x4 hq = __builtin_bit_cast(u32x4, rk0[i][ps]), lq = __builtin_bit_cast(u32x4, rk1[i][ps]);
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
              const unsigned hw_ = hq[e2], lw_ = lq[e2];   // (a scalar copy first: __builtin_bit_cast of a vector ELEMENT reads element 0 whatever the index -- hipcc 7.2)
              const f16x2 h2 = __builtin_bit_cast(f16x2, hw_), l2 = __builtin_bit_cast(f16x2, lw_);
              ev[2 * e2] += ((float)h2[0] + (float)l2[0] * kLoInv) * rsc;
              ev[2 * e2 + 1] += ((float)h2[1] + (float)l2[1] * kLoInv) * rsc;
            }
          } else if (resf) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { ev[e] += rk0[i][ps][e]; ev[4 + e] += rk1[i][ps][e]; }
          }
          if (hasemb) {
#pragma unroll
            for (int e = 0; e < 8; ++e) ev[e] += mv[e];
          }
          const long eo = (long)m * p.Cout + col0;
          if (p.fz.out_f32) {
            *reinterpret_cast<f32x4*>(p.fz.out_f32 + eo) = f32x4{ev[0], ev[1], ev[2], ev[3]};
            *reinterpret_cast<f32x4*>(p.fz.out_f32 + eo + 4) = f32x4{ev[4], ev[5], ev[6], ev[7]};
          }
          sf_u32x4 hi, lo;
          split8_f16<false>(sf_f32x4{ev[0] * osc, ev[1] * osc, ev[2] * osc, ev[3] * osc}, sf_f32x4{ev[4] * osc, ev[5] * osc, ev[6] * osc, ev[7] * osc}, hi, lo);
          sf_u32x4* op = reinterpret_cast<sf_u32x4*>(reinterpret_cast<char*>(p.fz.out_pairs) + (eo >> 3) * 32);
          op[0] = hi;
          op[1] = lo;
        }
      }
  }
