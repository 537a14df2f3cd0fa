// csg_amodal_tri.inc -- one triangle of a chunk through k_setup's per-triangle arithmetic for the
// amodal passes, included as text inside amodal_pass (csg_kernels.hip) and k_amodal_plane
// (csg_amodal_spans.hip): one source for both, and k_amodal / k_amodal_depth compile to the
// instructions they always had (as a function template with the sample rectangle as a functor the
// same arithmetic came out in another schedule).  The includer provides
//   s (SceneDev), a (.iset [sets][instances]), clipm[12] (rows 0, 1, 3 of P * (V * M)), ch (Chunk),
//   tid, set, inst, and the macros CSG_AM_COL(v) / CSG_AM_ROW(v): the first sample column / row
//   that lies on a pixel >= v (a record's inclusive pixel box [bx0, bx1] x [by0, by1] becomes the
//   sample rectangle [COL(bx0), COL(bx1 + 1)) x [ROW(by0), ROW(by1 + 1))),
// and gets t0 (, t1): the raster sub-triangles with their sample rectangles, and nrec = 0, 1 or 2.
  // k_setup's per-triangle arithmetic (setup_chunk), kept in the same order
  AmTri t0 = {}, t1 = {};
  int nrec = 0;
  if ((uint32_t)tid < ch.count) {
    const uint32_t g = ch.soup + tid;
    Cv3 v[3];
    float c[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) c[q] = clipm[q];
    const float* tp = s.tri_pos + (size_t)g * 9;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float px = tp[3 * q], py = tp[3 * q + 1], pz = tp[3 * q + 2];
      v[q].x = dot4(c + 0, px, py, pz);
      v[q].y = dot4(c + 4, px, py, pz);
      v[q].w = dot4(c + 8, px, py, pz);
    }
    const float nearc = s.near_clip, farc = s.far_clip;
    const float Wf = (float)s.W, Hf = (float)s.H;
    bool on = true, of = true, ol = true, orr = true, ot = true, ob = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      on &= v[q].w < nearc;
      of &= v[q].w > farc;
      ol &= v[q].x < 0.0f;
      orr &= v[q].x > Wf * v[q].w;
      ot &= v[q].y < 0.0f;
      ob &= v[q].y > Hf * v[q].w;
    }
    if (!(on | of | ol | orr | ot | ob)) {
      Cv3 q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[2];
      int nq = 3;
      const bool in0 = v[0].w >= nearc, in1 = v[1].w >= nearc, in2 = v[2].w >= nearc;
      if (!(in0 && in1 && in2)) {
        auto cross_pt = [&](const Cv3& p, const Cv3& bb) {
          const float tt = (nearc - p.w) / (bb.w - p.w);
          Cv3 rr;
          rr.x = p.x + tt * (bb.x - p.x);
          rr.y = p.y + tt * (bb.y - p.y);
          rr.w = nearc;
          return rr;
        };
        auto sel = [](bool cnd, const Cv3& p, const Cv3& bb) {
          Cv3 rr;
          rr.x = cnd ? p.x : bb.x;
          rr.y = cnd ? p.y : bb.y;
          rr.w = cnd ? p.w : bb.w;
          return rr;
        };
        const Cv3 I01 = cross_pt(v[0], v[1]), I12 = cross_pt(v[1], v[2]), I20 = cross_pt(v[2], v[0]);
        const int code = (int)in0 | ((int)in1 << 1) | ((int)in2 << 2);
        q0 = sel(code == 2 || code == 6, I01, sel(code == 4, I12, v[0]));
        q1 = sel(code == 1 || code == 5, I01, sel(code == 4, v[2], v[1]));
        q2 = sel(code == 1 || code == 4, I20, sel(code == 6, v[2], I12));
        q3 = sel(code == 3 || code == 6, I20, v[2]);
        nq = (code == 1 || code == 2 || code == 4) ? 3 : 4;
      }
      // a sub-triangle's record, then the samples of the window inside its pixel box
      auto emit_tri = [&](const Cv3& p, const Cv3& bb, const Cv3& cc) {
        const float ra = rcp_w(p.w), rb = rcp_w(bb.w), rc = rcp_w(cc.w);
        float su[3], sv[3];
        su[0] = p.x * ra; sv[0] = p.y * ra;
        su[1] = bb.x * rb; sv[1] = bb.y * rb;
        su[2] = cc.x * rc; sv[2] = cc.y * rc;
        SubRec rr;
        if (!make_rec(s, su, sv, rr)) return;
        const int32_t bx0 = (int32_t)(rr.g1.z & 0xFFFFu), by0 = (int32_t)(rr.g1.z >> 16);
        const int32_t bx1 = (int32_t)(rr.g1.w & 0xFFFFu), by1 = (int32_t)(rr.g1.w >> 16);
        const uint32_t i0 = CSG_AM_COL(bx0), i1 = CSG_AM_COL(bx1 + 1);
        if (i0 >= i1) return;
        const uint32_t j0 = CSG_AM_ROW(by0), j1 = CSG_AM_ROW(by1 + 1);
        if (j0 >= j1) return;
        // into t0, then t1: selects on named structs, never a runtime-chosen one (as k_setup's r0, r1)
        const bool first = nrec == 0;
        auto put = [](AmTri& d, bool on, const SubRec& r, uint32_t a0, uint32_t an, uint32_t b0, uint32_t bn) {
          d.x[0] = on ? (int32_t)r.g0.x : d.x[0]; d.x[1] = on ? (int32_t)r.g0.y : d.x[1];
          d.x[2] = on ? (int32_t)r.g0.z : d.x[2]; d.y[0] = on ? (int32_t)r.g0.w : d.y[0];
          d.y[1] = on ? (int32_t)r.g1.x : d.y[1]; d.y[2] = on ? (int32_t)r.g1.y : d.y[2];
          d.i0 = on ? a0 : d.i0; d.ni = on ? an : d.ni; d.j0 = on ? b0 : d.j0; d.nj = on ? bn : d.nj;
        };
        put(t0, first, rr, i0, i1 - i0, j0, j1 - j0);
        put(t1, !first, rr, i0, i1 - i0, j0, j1 - j0);
        ++nrec;
      };
      if (nq >= 3) emit_tri(q0, q1, q2);
      if (nq >= 4) emit_tri(q0, q2, q3);
      if (nrec > 0) {
        Hom h;
        hom_setup(v, h);
        const InstSetDev is = a.iset[(size_t)set * s.n_inst + inst];
        // as k_setup: no record without a determinant, none under a threshold of 255
        if (!h.ok || (is.atex != kNoAlpha && is.athr >= 255u)) {
          nrec = 0;
        } else {
          float D[3], U[3] = {0.0f, 0.0f, 0.0f}, V[3] = {0.0f, 0.0f, 0.0f};
          depth_plane(h.A, h.B, h.C, h.invdet, D);
          if (is.alpha_uv) {
            const float* tu = s.tri_uv + (size_t)g * 6;
            float uv[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) uv[q] = tu[q];
            uv_planes(h.A, h.B, h.C, h.invdet, uv, U, V);
          }
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            t0.D[q] = t1.D[q] = D[q];
            t0.U[q] = t1.U[q] = U[q];
            t0.V[q] = t1.V[q] = V[q];
          }
          t0.atex = t1.atex = is.atex;
          t0.wh = t1.wh = is.atex_wh;
          t0.thr = t1.thr = is.athr;
        }
      }
    }
  }
