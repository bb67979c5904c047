// tf_ff_distal.inc - the distal finger-finger pass: the pairs (0,1), (1,2), (2,0) in turn, one frictionless normal row each, resolved before the sweeps
// on the free velocities, which live in LDS (L_VQFF) while the pairs are visited.  Reads what the fingers published before S1 (LDS only) - run by the
// cube role between S1 and S1b (tf_roles.h includes it there and nowhere else); in the instantiation with helper wavefronts, wavefront 7 runs the same
// rows in a layout of its own (helper_role).  Textual inclusion; uses m, h, inv_h, rest_ff, lds, lane.
#pragma unroll
            for (int f = 0; f < 3; ++f) {
#pragma unroll
                for (int j = 0; j < 3; ++j) LD(L_VQFF + 3 * f + j) = LD(L_REC(f) + P_VQ + j);
            }
#pragma unroll 1                                                // (unrolling the three pairs in the 256-register build changes nothing: measured)
            for (int p = 0; p < 3; ++p) {
                const int fa = p, fb = (p == 2) ? 0 : p + 1;
                float Pa[3], Pb[3];
                {
                    float Aa[3], Ba[3], Ab[3], Bb[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) { Aa[j] = LD(L_REC(fa) + P_AW + j); Ba[j] = LD(L_REC(fa) + P_BW + j); Ab[j] = LD(L_REC(fb) + P_AW + j); Bb[j] = LD(L_REC(fb) + P_BW + j); }
                    seg_seg(Aa, Ba, Ab, Bb, Pa, Pb);
                }
                float dv[3] = {Pa[0] - Pb[0], Pa[1] - Pb[1], Pa[2] - Pb[2]};
                float dist2 = dot3(dv, dv);
                float inv = f_rsqrt(f_max(dist2, 1e-12f));
                float dist = dist2 * inv;
                float gap = dist - 2.0f * m.cap_radius;
                if ((dist2 > 1e-12f) && (gap < m.contact_margin)) {
                    float n[3] = {dv[0] * inv, dv[1] * inv, dv[2] * inv};       // from finger b to finger a
                    float Ja[3], Wa[3], Jb[3], Wb[3], va[3], vb[3];
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const int ff_ = side ? fb : fa;
                        const Yaw yy = {m.base_yaw_cos[ff_], m.base_yaw_sin[ff_], 0.0f, 0.0f, m.base_height};
                        FingerPubRegs pp;
                        read_pub<WIDE>(m, lds, lane, ff_, pp);
                        float C[3], Cb_[3], L1[3], L2[3], L3[3], nb[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) C[j] = side ? FMA(m.cap_radius, n[j], Pb[j]) : FMA(-m.cap_radius, n[j], Pa[j]);
                        world_to_base(yy, C, Cb_);
                        levers(pp.k, Cb_, L1, L2, L3);
                        dir_world_to_base(yy, n, nb);
                        float* J = side ? Jb : Ja;
                        float* W = side ? Wb : Wa;
                        float* vv = side ? vb : va;
                        J[0] = dot3(L1, nb); J[1] = dot3(L2, nb); J[2] = dot3(L3, nb);
                        sym3_mul(pp.k.Minv, J, W);
#pragma unroll
                        for (int j = 0; j < 3; ++j) vv[j] = LD(L_VQFF + 3 * ff_ + j);
                    }
                    float vn0 = dot3(Ja, va) - dot3(Jb, vb);
                    if (contact_live(m, gap, vn0, h)) {
                        float lam = ff_lambda(m, gap, vn0, inv_h, rest_ff, Ja, Wa, Jb, Wb);
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            LD(L_VQFF + 3 * fa + j) = FMA(Wa[j], lam, va[j]);
                            LD(L_VQFF + 3 * fb + j) = FMA(-Wb[j], lam, vb[j]);
                        }
                    }
                }
            }
