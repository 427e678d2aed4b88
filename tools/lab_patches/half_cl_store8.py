"""Kernel lab (not product code; ``tools/build_variant_lib.py`` patch): ``gemm_cl_half``'s first epilogue, one
8-byte store per 16 x 16 tile (a lane's four accumulator registers are four consecutive channels of its pixel:
16 stores per lane for the wave's 64 x 64, the four lanes of a pixel writing 32 contiguous bytes per
instruction), where the product kernel transposes the wave's four 16-channel blocks across the four lanes of a
pixel and issues two 16-byte stores per column tile (8 per lane, 128 contiguous bytes per pixel).  Outputs
bit-identical.  Measured in one process, the two forms taking turns call by call (``tools/ab_half_nn.py
<variant>.so 50 cl``, medians of 50, us, 8-byte form vs product): configs[1] bf16 forward 197.7 vs 178.3, data
gradient 238.5 vs 214.0; fp16 202.3 vs 182.5, 258.7 vs 217.6; configs[2] bf16 148.9 vs 137.9, 139.2 vs 119.8;
fp16 151.5 vs 140.7, 144.0 vs 124.8; configs[4] bf16 167.5 vs 147.5, 190.0 vs 155.5; fp16 170.6 vs 150.4, 192.5
vs 158.7 - the product form takes 0.88-0.93 x the 8-byte form's time in the forward and 0.82-0.90 x in the data
gradient, on every row.  The 8-byte form is not applied."""
PATCH = [
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
  char* po0[4];
  char* po1[4];
  bool live[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int64_t n = nbase + 64 * wn + 16 * ni + r16;
    live[ni] = n < a.nrows;
    const uint32_t nn = (uint32_t)(live[ni] ? n : 0);
    const uint32_t nd = nn / (uint32_t)a.P, px = nn - nd * (uint32_t)a.P;
    po0[ni] = a.c0 + 2 * ((int64_t)nd * a.c0n + (int64_t)px * a.c0p + 4 * qq);
    po1[ni] = a.c1 + 2 * ((int64_t)nd * a.c1n + (int64_t)px * a.c1p + 4 * qq);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mrow = mb0 + 16 * mi;
    if (mrow >= a.M) continue;
    const bool side1 = mrow >= a.m0;
    const int srow = side1 ? mrow - a.m0 : mrow;
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr) {
      const float* bp = a.bias + mrow + 4 * qq;
      bv = {bp[0], bp[1], bp[2], bp[3]};
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      if (!live[ni]) continue;
      f4 v = acc[mi][ni];
      if (a.bias != nullptr) v = v + bv;
      const typename T::v4 e = __builtin_convertvector(v, typename T::v4);
      *reinterpret_cast<u2*>((side1 ? po1[ni] : po0[ni]) + 2 * srow) = __builtin_bit_cast(u2, e);
    }
  }
}
'''),
]
