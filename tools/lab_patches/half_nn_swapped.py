"""Kernel lab (not product code; ``tools/build_variant_lib.py`` patch): ``gemm_nn_half`` with the MFMA's
operand roles swapped (activation rows x weight columns), so a lane's four accumulator registers are four
consecutive pixels of one channel and the epilogue issues one 8-byte ``buffer_store_dwordx2`` per tile
after ``v_cvt_pk_{bf16,f16}_f32`` (16 stores per lane for the wave's 64 x 64) where the product kernel
issues one 2-byte store per register (64 per lane).  Outputs bit-identical.  Measured against the product
form in one process, the two taking turns call by call (``tools/ab_half_nn.py``, medians of 50, us,
swapped vs product): configs[1] bf16 forward 187.7 vs 178.6, data gradient 232.1 vs 213.2; fp16 192.7 vs
185.6, 233.4 vs 214.8; configs[2] bf16 152.3 vs 150.3, 125.3 vs 122.4; fp16 154.7 vs 152.3, 131.7 vs 127.4;
configs[4] bf16 157.6 vs 154.5, 172.7 vs 162.3; fp16 161.9 vs 157.6, 178.1 vs 166.9 - the swapped form is
2-8 % slower on every row although it issues a quarter of the store instructions.  Not applied."""
PATCH = [
    ('compress_half.hip', '''acc[mi][ni] = T::mma(ar[mi], bf[ni], acc[mi][ni]);  // channels x pixels''',
     '''acc[mi][ni] = T::mma(bf[ni], ar[mi], acc[mi][ni]);  // pixels x channels'''),
    ('compress_half.hip', '''  const int mb0 = mt * TM + 64 * wm;
  uint32_t vo0[4], vo1[4];  // per ni: byte offset of (node, pixel, row 4 qq) in c0 / c1
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    const bool live = n < a.ncols;
    const uint32_t nn = (uint32_t)(live ? n : 0);
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    vo0[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c0s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
    vo1[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c1s) + px + (uint32_t)(4 * qq * a.P)) : 0x80000000u;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    if (mrow >= a.M) continue;
    const bool side1 = mrow >= a.m0;
    const uint32_t srow = (uint32_t)(side1 ? mrow - a.m0 : mrow);
    const __amdgpu_buffer_rsrc_t rc = rsrc(side1 ? a.c1 : a.c0);
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr) {
      const float* bp = a.bias + mrow + 4 * qq;
      bv = {bp[0], bp[1], bp[2], bp[3]};
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t so = 2u * (srow + (uint32_t)r) * (uint32_t)a.P;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        float v = acc[mi][ni][r];
        if (a.bias != nullptr) v = v + bv[r];
        const typename T::elem e = (typename T::elem)v;
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, e), rc, side1 ? vo1[ni] : vo0[ni], so, 0);
      }
    }
  }
}

''',
     '''  const int mb0 = mt * TM + 64 * wm;
  uint32_t vo0[4], vo1[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + 4 * qq;
    const bool live = n < a.ncols;  // ncols % 4 == 0: the four pixels are live together
    const uint32_t nn = (uint32_t)(live ? n : 0);  // the launch requires ncols < 2^31
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    vo0[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c0s) + px + (uint32_t)(r16 * a.P)) : 0x80000000u;
    vo1[ni] = live ? 2u * ((uint32_t)((int64_t)nd * a.c1s) + px + (uint32_t)(r16 * a.P)) : 0x80000000u;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;  // the block's first row (wave-uniform)
    if (mrow >= a.M) continue;
    const bool side1 = mrow >= a.m0;
    const uint32_t so = 2u * (uint32_t)(side1 ? mrow - a.m0 : mrow) * (uint32_t)a.P;
    const __amdgpu_buffer_rsrc_t rc = rsrc(side1 ? a.c1 : a.c0);
    const float bv = a.bias != nullptr ? a.bias[mrow + r16] : 0.f;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      f4 o = acc[mi][ni];
      if (a.bias != nullptr) o = o + bv;
      const u2 pk = __builtin_bit_cast(u2, __builtin_convertvector(o, typename T::v4));
      __builtin_amdgcn_raw_buffer_store_b64(pk, rc, side1 ? vo1[ni] : vo0[ni], so, 0);
    }
  }
}

'''),
]
