// tf_wall_corners.inc - the cube role's boundary-corner block (tf_roles.h includes it at the place the instantiation builds these rows: before S1, or -
// with helper wavefronts, where another wavefront runs the distal finger-finger pass - between S1 and S1b).  Textual inclusion, as tf_floor_corners.inc.
// Uses the cube role's locals: R, hc, cp, v, w, h, inv_h, inv_m, inv_I, ws, m, box, soff, cw_face, P, lds, lane; fills wall_lane, slot_any, cw_face, the
// rows in LDS (L_WALL) and - WREG - w_r, w_n, w_D, w_bias, w_lam, w_a, w_b; SURF (TfModel.cube_wall_surface): a corner above wall_z[0] gets the rows of
// the tilted surface instead (L_CONE, cone_any) and its ring rows stay dead.  A corner on the vertical ring takes the same path with or without SURF.
            {   // cube vs boundary wall: the four corners of the face that points outward most; rows go to LDS
                const float cx_ = EXT ? cp[0] - soff[0] : cp[0], cy_ = EXT ? cp[1] - soff[1] : cp[1];      // relative to the stage centre
                float rc2 = FMA(cx_, cx_, cy_ * cy_);
                float irc = f_rsqrt(f_max(rc2, 1e-24f));
                float rho_c = rc2 * irc;
                bool any = rho_c > 1e-6f;
                float dx = 0.0f, dy = 0.0f;
                if (any) { dx = cx_ * irc; dy = cy_ * irc; }
                float pr[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) pr[j] = FMA(R[j], dx, R[3 + j] * dy);
                int k = 0;
                float out[3] = {f_abs(pr[0]), f_abs(pr[1]), f_abs(pr[2])};
                if (__builtin_expect(box, 0)) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) out[j] = out[j] * hc[j];
                }
                float best = out[0];
                if (out[1] > best) { best = out[1]; k = 1; }
                if (out[2] > best) { best = out[2]; k = 2; }
                float pk = (k == 0) ? pr[0] : ((k == 1) ? pr[1] : pr[2]);
                float sk = (pk < 0.0f) ? -1.0f : 1.0f;
                // Slot order of the four corners: the LOWER pair of the face first (slots 0, 1), the upper pair behind it.  A cube that lies at
                // the boundary touches it with its lower pair, so the lanes of a wavefront agree on which slots are live and the sweeps run two
                // corner blocks instead of up to four (the step ends with its slowest workgroup: DESIGN.md section 4).  With a < b the two axes of
                // the face, the "heavy" one is the axis whose corner offset has the larger vertical component; the pair is chosen by its sign,
                // inside the lower pair the corner nearer to the boundary comes first (a cube usually touches the concave wall with one corner: it
                // then sits in slot 0 in every lane), decided anew in every substep - the warm-start rows follow their corner when the order of
                // the pair changes; the upper pair is ordered by the sign along the other axis.  The feature the warm start is keyed by is
                // face + 8 x pair, stored with the order: + 32 x order.
                const int a_ = (k == 0) ? 1 : 0, b_ = (k == 2) ? 1 : 2;
                const float wa_ = hc[a_] * ((a_ == 0) ? R[6] : R[7]), wb_ = hc[b_] * ((b_ == 1) ? R[7] : R[8]);
                const bool heavy_b = f_abs(wb_) > f_abs(wa_);
                const int lowh = ((heavy_b ? wb_ : wa_) < 0.0f) ? 1 : 0;      // sign bit of the heavy axis that points down
                const float face_pair = (float)(2 * k + 1 + ((sk > 0.0f) ? 1 : 0) + 8 * ((heavy_b ? 2 : 0) + lowh));
                int order, swap01;
                float keep, lam_old[6];
                {
                    const float prev_o = (cw_face >= 32.0f) ? 1.0f : 0.0f;
                    float gl[2];
#pragma unroll
                    for (int lb = 0; lb < 2; ++lb) {             // horizontal gap of the two corners of the lower pair
                        float rr[3];
                        cube_corner(R, hc, k, sk, heavy_b ? (lb | (lowh << 1)) : (lowh | (lb << 1)), rr);
                        const float qx = cx_ + rr[0], qy = cy_ + rr[1];
                        const float q2 = FMA(qx, qx, qy * qy);
                        gl[lb] = wall_radius_at(P, cp[2] + rr[2]) - q2 * f_rsqrt(f_max(q2, 1e-24f));
                    }
                    order = (gl[1] < gl[0]) ? 1 : 0;
                    swap01 = order ^ (int)prev_o;
                    keep = (FMA(-32.0f, prev_o, cw_face) == face_pair) ? ws : 0.0f;
#pragma unroll
                    for (int j = 0; j < 6; ++j) lam_old[j] = LD(L_WALL + 12 * (j / 3) + 9 + (j % 3));      // slots 0 and 1 before they are rewritten
                }
                const float face = FMA(32.0f, (float)order, face_pair);
                wall_lane = false;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int wb = L_WALL + 12 * c;
                    float r[3], n[2] = {0.0f, 0.0f}, Dinv[3] = {0.0f, 0.0f, 0.0f}, bias = 0.0f, lam[3] = {0.0f, 0.0f, 0.0f};
                    const int hbit = (c >> 1) ^ lowh, lbit = (c < 2) ? ((c & 1) ^ order) : (c & 1);
                    cube_corner(R, hc, k, sk, heavy_b ? (lbit | (hbit << 1)) : (hbit | (lbit << 1)), r);
                    float px = cx_ + r[0], py = cy_ + r[1], pz = cp[2] + r[2];
                    float rho2 = FMA(px, px, py * py);
                    float inv = f_rsqrt(f_max(rho2, 1e-24f));
                    float rho = rho2 * inv;
                    float gap, wc = 1.0f, wsn = 0.0f;
                    bool cone = false, cone_live = false;       // SURF: the corner is above the vertical ring / has live rows of the tilted surface
                    float cone_lam[3] = {0.0f, 0.0f, 0.0f}, cone_D0 = 0.0f;
                    if constexpr (SURF) {
                        const float rz = wall_profile(P, pz, wc, wsn);
                        cone = pz > m.wall_z[0];
                        gap = cone ? (rz - rho) * wc : rz - rho;     // distance to the tilted surface; on the ring the horizontal gap as below
                    } else {
                        gap = wall_radius_at(P, pz) - rho;
                    }
                    if (__builtin_expect(any && gap < m.contact_margin && rho > 1e-6f, 0)) {
                        float nn[2] = {-px * inv, -py * inv};
                        if (SURF && cone) {                     // rows N, T, U of the surface (general rows; the slot's ring rows stay dead)
                            float dd[9], aa[9];
                            surface_rows(r, nn, wc, wsn, dd, aa);
                            const float vn0 = g_vrel(&dd[0], &aa[0], v, w);
                            if (contact_live(m, gap, vn0, h)) {
                                cone_live = true;
                                const int cb = L_CONE + 22 * c;
#pragma unroll
                                for (int j = 0; j < 9; ++j) { LD(cb + 6 * (j / 3) + j % 3) = dd[j]; LD(cb + 6 * (j / 3) + 3 + j % 3) = aa[j]; }
                                cone_D0 = f_rcp2(FMA(dot3(&aa[0], &aa[0]), inv_I, inv_m));
                                LD(cb + 19) = f_rcp2(FMA(dot3(&aa[3], &aa[3]), inv_I, inv_m));
                                LD(cb + 20) = f_rcp2(FMA(dot3(&aa[6], &aa[6]), inv_I, inv_m));
                                LD(cb + 21) = contact_bias(m, gap, vn0, inv_h, 0.0f);
#pragma unroll
                                for (int d = 0; d < 3; ++d) cone_lam[d] = ((c < 2) ? (((c ^ swap01) == 0) ? lam_old[d] : lam_old[3 + d]) : LD(wb + 9 + d)) * keep;
                            }
                        } else {
                        float a[3], b[3], c3[3];
                        wall_arms(box, lds, lane, r, nn, a, b, c3);
                        const float vn0 = wn_vrel(nn, a, v, w);
                        if (contact_live(m, gap, vn0, h)) {
                            n[0] = nn[0]; n[1] = nn[1];
                            Dinv[0] = f_rcp2(FMA(dot3(a, a), inv_I, inv_m));
                            Dinv[1] = f_rcp2(FMA(dot3(b, b), inv_I, inv_m));
                            Dinv[2] = box ? f_rcp2(FMA(dot3(c3, c3), inv_I, inv_m)) : f_rcp2(FMA(FMA(r[0], r[0], r[1] * r[1]), inv_I, inv_m));
                            bias = contact_bias(m, gap, vn0, inv_h, 0.0f);
#pragma unroll
                            for (int d = 0; d < 3; ++d) lam[d] = ((c < 2) ? (((c ^ swap01) == 0) ? lam_old[d] : lam_old[3 + d]) : LD(wb + 9 + d)) * keep;
                        }
                        }
                    }
                    if constexpr (SURF) LD(L_CONE + 22 * c + 18) = cone_D0;        // 0 unless live: the sweeps test the lane's 1/D of N
                    if (WREG && c < 2) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) { w_r[3 * c + j] = r[j]; w_D[3 * c + j] = Dinv[j]; w_lam[3 * c + j] = lam[j]; LD(wb + 9 + j) = lam[j]; }
                        w_n[2 * c] = n[0]; w_n[2 * c + 1] = n[1]; w_bias[c] = bias;
                        wall_arm_n(r, n, &w_a[3 * c]);
                        wall_arm_t(r, n, &w_b[3 * c]);
                    } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j) { LD(wb + j) = r[j]; LD(wb + 5 + j) = Dinv[j]; LD(wb + 9 + j) = lam[j]; }
                    LD(wb + 3) = n[0]; LD(wb + 4) = n[1]; LD(wb + 8) = bias;
                    }
                    wall_lane = wall_lane || (Dinv[0] > 0.0f);
                    slot_any[c] = __builtin_amdgcn_ballot_w64(Dinv[0] > 0.0f) != 0ull;
                    if constexpr (SURF) {
                        if (cone_live) {
#pragma unroll
                            for (int d = 0; d < 3; ++d) LD(wb + 9 + d) = cone_lam[d];     // the impulses live in the corner slot's rows
                        }
                        wall_lane = wall_lane || cone_live;
                        cone_any |= (__builtin_amdgcn_ballot_w64(cone_live) != 0ull) ? (1u << c) : 0u;
                    }
                }
                cw_face = wall_lane ? face : 0.0f;              // 0: no corner touches the boundary (the rows carry nothing)
            }
