"""Kernel lab (not product code; ``tools/build_variant_lib.py`` patch): ``gemm_cl_half`` with the MFMA's
operand roles swapped (pixel rows x weight columns), so a lane's four accumulator registers are four
consecutive pixel rows of one channel and the epilogue issues one 2-byte store per register (64 per lane
for the wave's 64 x 64, sixteen lanes writing 32 contiguous bytes of a pixel row) where the product kernel
keeps the weight as the row operand and, after a transpose across the four lanes of a pixel, issues two
16-byte stores per column tile (8 per lane, 128 contiguous bytes per pixel).  Outputs bit-identical.  Timed by
``tools/ab_half_nn.py <variant>.so 50 cl`` (medians of 50, us) against the weight-rows form with one 8-byte
store per tile (``half_cl_store8.py``), 8-byte form vs swapped: configs[1] bf16 forward 192.4 vs 199.4, data
gradient 235.8 vs 260.7; fp16 196.8 vs 201.6, 257.3 vs 260.7; configs[2] bf16 148.5 vs 148.5, 139.9 vs 136.7;
fp16 152.4 vs 152.4, 144.8 vs 140.9; configs[4] bf16 165.6 vs 159.4, 185.2 vs 178.9; fp16 171.2 vs 163.6, 191.1
vs 181.8 - 0.95-1.10, no winner across shapes; the product's 16-byte stores, which these roles cannot have,
beat both.  Not applied."""
PATCH = [
    ('compress_half_cl.hip', '''acc[mi][ni] = T::mma(ar[mi], bf[ni], acc[mi][ni]);  // channels x pixels''',
     '''acc[mi][ni] = T::mma(bf[ni], ar[mi], acc[mi][ni]);  // pixels x channels'''),
    ('compress_half_cl.hip', '''  const int mb0 = mt * TM + 64 * wm;
  const int mg = mb0 + 16 * qq;  // the lane's 16 channels after the transpose
  const bool glive = mg < a.M, gside1 = mg >= a.m0;
  const int gs = gside1 ? mg - a.m0 : mg;
  f4 bv[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    bv[mi] = f4{0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr && mrow < a.M) {
      const float* bp = a.bias + mrow + 4 * qq;
      bv[mi] = f4{bp[0], bp[1], bp[2], bp[3]};
    }
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    const bool live = n < a.nrows;
    const uint32_t nn = (uint32_t)(live ? n : 0);
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    u2 piece[4], grp[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      f4 v = acc[mi][ni];
      if (a.bias != nullptr) v = v + bv[mi];
      piece[mi] = __builtin_bit_cast(u2, __builtin_convertvector(v, typename T::v4));
      grp[mi] = piece[mi];
    }
    // round s: lane qq sends its piece of block (qq - s) & 3 and takes, from lane (qq + s) & 3 of its pixel,
    // that lane's piece of block qq: channels 16 qq + 4 ((qq + s) & 3) ..  Every lane takes part (blocks
    // past M and rows past the end carry values that are never stored).
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      const int si = (qq - s) & 3, dj = (qq + s) & 3;
      const u2 snd = si == 0 ? piece[0] : si == 1 ? piece[1] : si == 2 ? piece[2] : piece[3];
      const int src = r16 + 16 * dj;
      const u2 rcv = {(uint32_t)__shfl((int)snd.x, src, 64), (uint32_t)__shfl((int)snd.y, src, 64)};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (dj == j) grp[j] = rcv;
    }
    // the lane's own piece of block qq belongs at position qq
    const u2 own = qq == 0 ? piece[0] : qq == 1 ? piece[1] : qq == 2 ? piece[2] : piece[3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (qq == j) grp[j] = own;
    if (live && glive) {
      char* p = (gside1 ? a.c1 + 2 * ((int64_t)nd * a.c1n + (int64_t)px * a.c1p)
                        : a.c0 + 2 * ((int64_t)nd * a.c0n + (int64_t)px * a.c0p)) + 2 * gs;
      *reinterpret_cast<u4*>(p) = u4{grp[0].x, grp[0].y, grp[1].x, grp[1].y};
      *reinterpret_cast<u4*>(p + 16) = u4{grp[2].x, grp[2].y, grp[3].x, grp[3].y};
    }
  }
}
''',
     '''  const int mb0 = mt * TM + 64 * wm;
  float bv[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    bv[mi] = a.bias != nullptr && mrow < a.M ? a.bias[mrow + r16] : 0.f;
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n0 = nbase + 64 * wn + 16 * ni + 4 * qq;
    if (n0 >= a.nrows) continue;
    const uint32_t nd0 = (uint32_t)n0 / (uint32_t)a.P, px0 = (uint32_t)n0 - nd0 * (uint32_t)a.P;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (n0 + r >= a.nrows) continue;
      uint32_t px = px0 + r, nd = nd0;
      while (px >= (uint32_t)a.P) {
        px -= (uint32_t)a.P;
        ++nd;
      }
      char* p0 = a.c0 + 2 * ((int64_t)nd * a.c0n + (int64_t)px * a.c0p + r16);
      char* p1 = a.c1 + 2 * ((int64_t)nd * a.c1n + (int64_t)px * a.c1p + r16);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int mrow = mb0 + 16 * mi;
        if (mrow >= a.M) continue;
        const bool side1 = mrow >= a.m0;
        const int srow = side1 ? mrow - a.m0 : mrow;
        float v = acc[mi][ni][r];
        if (a.bias != nullptr) v = v + bv[mi];
        const typename T::elem e = (typename T::elem)v;
        *reinterpret_cast<typename T::elem*>((side1 ? p1 : p0) + 2 * srow) = e;
      }
    }
  }
}
'''),
]
