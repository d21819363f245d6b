// Planar kinematic trees with ground contact on device beside envs.h's Hopper (fp64, FMA
// contraction off), operation-for-operation twin of tests/halfcheetah_np.py: HalfCheetah-v2,
// the "cheetah" task of the reference's MuJoCo battery.  gym and MuJoCo are absent, so parity
// with them is unpinned, as Hopper's is; the model restates gym's half_cheetah.xml and this
// header is the record of every constant.  No multiply-add is fused here (no fmad call): the
// twin is plain numpy, and only sin / cos / log / sqrt may differ from it in the last bit.
//
// The dynamics are written once (tree_substep) over a constant table (TreeTable) with a parent
// index per body; HalfCheetah is the first table.  Bodies 0 .. NB-1, parent[b] < b.  Body 0
// hangs on the joints rootx, rootz (slides) and rooty (hinge); body b >= 1 hangs on hinge b of
// its parent: q = (rootx, rootz, rooty, hinge 1 .. hinge NB-1).  Hinges turn about +y, a
// positive angle turns +z towards +x (envs_chains.h's convention); sgn[b] = -1 turns hinge b
// the other way (Hopper's hinges, which the twin steps through this code against
// oracle/envs.py).  A body-frame offset (u, w) at absolute angle phi is the world vector
// (u cos phi + w sin phi, w cos phi - u sin phi).
//
// Formulation: J^T A J in the absolute angles phi_b = phi_parent + sgn_b q_b.  Per body two
// constants of its own frame, from the table at compile time:
//     sa_b = m_b c_b + sum over children ch of (subtree mass of ch) (hinge of ch in b's frame)
//     jc_b = I_b + m_b |c_b|^2 + sum over children ch of (subtree mass of ch) |hinge of ch|^2
// and two world vectors per substep, S_b = sa_b turned by phi_b and G_b = (hinge of b in its
// parent's frame) turned by phi_parent.  In (x, z, phi_0 .. phi_NB-1) the kinetic energy has
//     A_xx = A_zz = total mass      A_x,b = S_b,z      A_z,b = -S_b,x      A_b,b = jc_b
//     A_a,d = G_c . S_d   for a an ancestor of d, c a's child on the way to d; 0 for bodies
//                         on different branches
// the velocity terms, with Y_ad = G_c,z S_d,x - G_c,x S_d,z,
//     c_x = -sum w_b^2 S_b,x    c_z = -sum w_b^2 S_b,z    c_d += w_a^2 Y_ad    c_a -= w_d^2 Y_ad
// and gravity Q_z = -M g, Q_b = g S_b,x.  A contact force f at a point of body b with lever o
// from b's hinge adds f to (Q_x, Q_z), o_z f_x - o_x f_z to Q_b and G_c,z F_x - G_c,x F_z to
// every ancestor (F: the subtree's force sum).  Sums over subtrees (children before parents)
// map the absolute-angle forces and inertia to the joints: r_b = sgn_b sum_subtree(b) Q,
// C_ab = sgn_a sgn_b sum_subtree(a) sum_subtree(b) A + armature, B0_b = sgn_b sum S_z,
// B1_b = -sgn_b sum S_x.  The translational block (total mass x identity) is eliminated by its
// Schur complement and the NB x NB rest solved by an LDL^T (7 x 7 for HalfCheetah);
// semi-implicit Euler: v += dt qdd, q += dt v.
//
// Forces on hinge b: gear_b clamp(a_b-1, -1, 1) - stiff_b q_b - damp_b qd_b + the one-sided
// penalty stops of Hopper's form at lo_b / hi_b (CH_KH, CH_CH).  Ground contact: Hopper's
// compliant contact unchanged (HP_KC, HP_CC, HP_CF) at the two end-spheres of every capsule,
// applied at the sphere's lowest point: depth pen = -(z of that point), normal force
// max(KC pen - CC v_z, 0) where pen > 0, friction -clamp(CF v_x, +-mu f_n).
//
// HalfCheetah-v2 (half_cheetah.xml).  Seven bodies in the x-z plane; the torso frame sits at
// z = 0.7 with rootz = 0 (the state stores the rootz offset, as gym's qpos).  Body frames in
// the parent's frame: bthigh (-0.5, 0) on the torso, bshin (0.16, -0.25), bfoot (-0.28, -0.14),
// fthigh (0.5, 0) on the torso, fshin (-0.14, -0.24), ffoot (0.13, -0.18).  Geoms: capsules of
// radius 0.046; the axis is the body's z turned about y by the angle, the centre in the body
// frame -- (half-length, angle, centre): torso (0.5, along x, (0, 0)), head on the torso body
// (0.15, 0.87, (0.6, 0.1)), bthigh (0.145, -3.8, (0.1, -0.13)), bshin (0.15, -2.03,
// (-0.14, -0.07)), bfoot (0.094, -0.27, (0.03, -0.097)), fthigh (0.133, 0.52, (-0.07, -0.12)),
// fshin (0.106, -0.6, (0.065, -0.09)), ffoot (0.07, -0.6, (0.045, -0.07)).  The sines and
// cosines of these angles are constants formed by tr_sin / tr_cos (24 series terms; the twin
// takes the same steps).  Masses and inertias from the geoms at uniform density
// (ch_capsule_mass / ch_capsule_inertia), scaled so that the total is 14 kg (settotalmass);
// the torso body combines its two geoms by the parallel-axis theorem.  In kg and kg m^2:
//     torso 6.2502 / 0.89712 (com (0.1524, 0.0254))   bthigh 1.5435 / 0.016844
//     bshin 1.5874 / 0.018267   bfoot 1.0954 / 0.0063524   fthigh 1.4381 / 0.013740
//     fshin 1.2008 / 0.0082221   ffoot 0.88452 / 0.0035291
// Hinges (stiffness about angle 0, damping, range, gear), armature 0.1 on all six and 0 on the
// root joints, which have no stiffness, damping or limit:
//     bthigh 240, 6, [-0.52, 1.05], 120     bshin 180, 4.5, [-0.785, 0.785], 90
//     bfoot 120, 3, [-0.4, 0.785], 60       fthigh 180, 4.5, [-1, 0.7], 120
//     fshin 120, 3, [-1.2, 0.87], 60        ffoot 60, 1.5, [-0.5, 0.5], 30
// Control clamped to [-1, 1], gravity (0, -9.81), friction 0.4 on every sphere.  MuJoCo's
// timestep is 0.01 and frame_skip 5: one env step is 0.05 s, taken in HC_NSUB substeps of
// HC_DT (DESIGN 5d has the study that chose it); the substep loop stays rolled.
// State (18) = q ++ qd.  obs (17) = q[1:] ++ qd, not clipped.  reward = (x_after - x_before) /
// 0.05 - 0.1 sum a^2 with the unclipped action.  done: never; TimeLimit 1000.  Reset (NU = 20
// uniforms): u0..u8 -> q = U(-0.1, 0.1), u9 unused, the pairs (u10, u11) .. (u18, u19) ->
// Box-Muller normals of oracle/philox.py, nine of the ten -> qd = 0.1 N(0, 1).
//
// Deviations from MuJoCo, documented like Hopper's:
//  * ground contact is the compliant sphere model above instead of the constraint solver, at
//    the capsules' end-spheres only (a capsule lying flat touches at its two ends);
//  * joint limits are one-sided penalty spring-dampers instead of the constraint solver;
//  * joint damping and stiffness are integrated explicitly (MuJoCo: implicitly in the
//    velocity), in substeps of HC_DT instead of one 0.01 step;
//  * geoms do not collide with each other (the XML's contype / conaffinity pairs them only
//    with the floor anyway).
#pragma once
#include "envs.h"
#include "envs_chains.h"

#pragma clang fp contract(off)

namespace mrl {

// sine and cosine of a constant by 24 series terms (the twin takes the same steps)
constexpr double tr_sin(double a) {
  double t = a, s = a;
  for (int k = 1; k < 25; ++k) {
    t = -t * a * a / (double)((2 * k) * (2 * k + 1));
    s = s + t;
  }
  return s;
}
constexpr double tr_cos(double a) {
  double t = 1.0, s = 1.0;
  for (int k = 1; k < 25; ++k) {
    t = -t * a * a / (double)((2 * k - 1) * (2 * k));
    s = s + t;
  }
  return s;
}

template <int NB_, int NSPH_>
struct TreeTable {
  static constexpr int NB = NB_, NQ = NB_ + 2, NSPH = NSPH_, NPAIR = NB_ * (NB_ - 1) / 2;
  int parent[NB_] = {};
  double sgn[NB_] = {}, px[NB_] = {}, pz[NB_] = {};  // hinge b's sign and place in the parent's frame
  double comx[NB_] = {}, comz[NB_] = {}, mass[NB_] = {}, inertia[NB_] = {};
  double arm[NB_] = {}, stiff[NB_] = {}, damp[NB_] = {}, lo[NB_] = {}, hi[NB_] = {}, gear[NB_] = {};
  int sbody[NSPH_] = {};  // contact spheres: body, centre (u, w) in its frame, radius, friction
  double su[NSPH_] = {}, sw[NSPH_] = {}, srad[NSPH_] = {}, smu[NSPH_] = {};
  double mt = 0.0, z0 = 0.0, dt = 0.0;
  int nsub = 0;
  // derived (tr_derive)
  double msub[NB_] = {}, sax[NB_] = {}, saz[NB_] = {}, jc[NB_] = {};
  int npair = 0, pa[NPAIR] = {}, pd[NPAIR] = {}, pc[NPAIR] = {};  // (ancestor, descendant, the ancestor's child on the way)
};

template <int NB, int NSPH>
constexpr TreeTable<NB, NSPH> tr_derive(TreeTable<NB, NSPH> t) {
  for (int b = 0; b < NB; ++b) {
    t.msub[b] = t.mass[b];
    t.sax[b] = t.mass[b] * t.comx[b];
    t.saz[b] = t.mass[b] * t.comz[b];
    t.jc[b] = t.inertia[b] + t.mass[b] * (t.comx[b] * t.comx[b] + t.comz[b] * t.comz[b]);
  }
  for (int b = NB - 1; b > 0; --b) {
    const int a = t.parent[b];
    t.sax[a] = t.sax[a] + t.msub[b] * t.px[b];
    t.saz[a] = t.saz[a] + t.msub[b] * t.pz[b];
    t.jc[a] = t.jc[a] + t.msub[b] * (t.px[b] * t.px[b] + t.pz[b] * t.pz[b]);
    t.msub[a] = t.msub[a] + t.msub[b];
  }
  for (int d = 1; d < NB; ++d) {
    int c = d, a = t.parent[d];
    while (true) {
      t.pa[t.npair] = a;
      t.pd[t.npair] = d;
      t.pc[t.npair] = c;
      t.npair += 1;
      if (a == 0) break;
      c = a;
      a = t.parent[a];
    }
  }
  return t;
}

// ------------------------------------------------------------------ HalfCheetah-v2: the table
constexpr int HC_NB = 7, HC_NGEOM = 8, HC_NSPH = 16;
constexpr int HC_NS = 18, HC_NQ = 9, HC_OBS = 17, HC_ACT = 6, HC_NU = 20, HC_MAX_STEPS = 1000;
constexpr double HC_R = 0.046, HC_TOTAL = 14.0, HC_MU = 0.4, HC_Z0 = 0.7, HC_CTRL = 1.0;
constexpr double HC_STEP = 0.05;  // MuJoCo's timestep 0.01 x frame_skip 5
constexpr double HC_DT = 0.00125;  // 0.01 / 8
constexpr int HC_NSUB = 40;
constexpr int HC_GBODY[HC_NGEOM] = {0, 0, 1, 2, 3, 4, 5, 6};
constexpr double HC_GHALF[HC_NGEOM] = {0.5, 0.15, 0.145, 0.15, 0.094, 0.133, 0.106, 0.07};
constexpr double HC_GANG[HC_NGEOM] = {0.0, 0.87, -3.8, -2.03, -0.27, 0.52, -0.6, -0.6};  // [0]: along x
constexpr double HC_GX[HC_NGEOM] = {0.0, 0.6, 0.1, -0.14, 0.03, -0.07, 0.065, 0.045};
constexpr double HC_GZ[HC_NGEOM] = {0.0, 0.1, -0.13, -0.07, -0.097, -0.12, -0.09, -0.07};

constexpr TreeTable<HC_NB, HC_NSPH> hc_table() {
  TreeTable<HC_NB, HC_NSPH> t;
  const int parent[HC_NB] = {0, 0, 1, 2, 0, 4, 5};
  const double px[HC_NB] = {0.0, -0.5, 0.16, -0.28, 0.5, -0.14, 0.13};
  const double pz[HC_NB] = {0.0, 0.0, -0.25, -0.14, 0.0, -0.24, -0.18};
  const double stiff[HC_NB] = {0.0, 240.0, 180.0, 120.0, 180.0, 120.0, 60.0};
  const double damp[HC_NB] = {0.0, 6.0, 4.5, 3.0, 4.5, 3.0, 1.5};
  const double lo[HC_NB] = {0.0, -0.52, -0.785, -0.4, -1.0, -1.2, -0.5};
  const double hi[HC_NB] = {0.0, 1.05, 0.785, 0.785, 0.7, 0.87, 0.5};
  const double gear[HC_NB] = {0.0, 120.0, 90.0, 60.0, 120.0, 60.0, 30.0};
  for (int b = 0; b < HC_NB; ++b) {
    t.parent[b] = parent[b];
    t.sgn[b] = 1.0;
    t.px[b] = px[b];
    t.pz[b] = pz[b];
    t.arm[b] = b == 0 ? 0.0 : 0.1;
    t.stiff[b] = stiff[b];
    t.damp[b] = damp[b];
    t.lo[b] = lo[b];
    t.hi[b] = hi[b];
    t.gear[b] = gear[b];
  }
  // masses and inertias of the geoms at uniform density, scaled to the total
  double gm[HC_NGEOM] = {}, gi[HC_NGEOM] = {};
  for (int g = 0; g < HC_NGEOM; ++g) {
    gm[g] = ch_capsule_mass(HC_R, 2.0 * HC_GHALF[g]);
    gi[g] = ch_capsule_inertia(HC_R, 2.0 * HC_GHALF[g]);
  }
  double tot = gm[0];
  for (int g = 1; g < HC_NGEOM; ++g) tot = tot + gm[g];
  const double sc = HC_TOTAL / tot;
  for (int g = 0; g < HC_NGEOM; ++g) {
    gm[g] = gm[g] * sc;
    gi[g] = gi[g] * sc;
  }
  // the torso body: its own capsule and the head, by the parallel-axis theorem
  const double m0 = gm[0] + gm[1];
  const double cx = (gm[1] * 0.6) / m0, cz = (gm[1] * 0.1) / m0;
  t.mass[0] = m0;
  t.comx[0] = cx;
  t.comz[0] = cz;
  t.inertia[0] = (gi[0] + gi[1]) +
                 (gm[0] * (cx * cx + cz * cz) + gm[1] * ((0.6 - cx) * (0.6 - cx) + (0.1 - cz) * (0.1 - cz)));
  for (int b = 1; b < HC_NB; ++b) {
    t.mass[b] = gm[b + 1];
    t.inertia[b] = gi[b + 1];
    t.comx[b] = HC_GX[b + 1];
    t.comz[b] = HC_GZ[b + 1];
  }
  // the two end-spheres of each capsule
  for (int g = 0; g < HC_NGEOM; ++g) {
    const double ax = g == 0 ? 1.0 : tr_sin(HC_GANG[g]), az = g == 0 ? 0.0 : tr_cos(HC_GANG[g]);
    for (int n = 0; n < 2; ++n) {
      const int k = 2 * g + n;
      t.sbody[k] = HC_GBODY[g];
      t.su[k] = n == 0 ? HC_GX[g] + HC_GHALF[g] * ax : HC_GX[g] - HC_GHALF[g] * ax;
      t.sw[k] = n == 0 ? HC_GZ[g] + HC_GHALF[g] * az : HC_GZ[g] - HC_GHALF[g] * az;
      t.srad[k] = HC_R;
      t.smu[k] = HC_MU;
    }
  }
  t.mt = HC_TOTAL;
  t.z0 = HC_Z0;
  t.dt = HC_DT;
  t.nsub = HC_NSUB;
  return tr_derive(t);
}
struct HcModel {
  static constexpr TreeTable<HC_NB, HC_NSPH> T = hc_table();
};

// ------------------------------------------------------------------ the tree dynamics
// one dt of the tree M::T under the hinge torques tau[NB - 1] (the motors'), semi-implicit Euler
template <class M>
__device__ inline void tree_substep(double* q, double* v, const double* tau) {
  constexpr int NB = M::T.NB, NQ = M::T.NQ, NSPH = M::T.NSPH, NPAIRS = M::T.npair;  // pairs in use (<= NPAIR slots)
  // absolute angles and rates, the world vectors S and G
  double phi[NB], om[NB], sn[NB], cs[NB];
  phi[0] = q[2];
  om[0] = v[2];
#pragma unroll
  for (int b = 1; b < NB; ++b) {
    phi[b] = phi[M::T.parent[b]] + M::T.sgn[b] * q[2 + b];
    om[b] = om[M::T.parent[b]] + M::T.sgn[b] * v[2 + b];
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) sincos(phi[b], &sn[b], &cs[b]);
  double Sx[NB], Sz[NB], Gx[NB], Gz[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    Sx[b] = M::T.sax[b] * cs[b] + M::T.saz[b] * sn[b];
    Sz[b] = M::T.saz[b] * cs[b] - M::T.sax[b] * sn[b];
  }
  Gx[0] = 0.0;
  Gz[0] = 0.0;
#pragma unroll
  for (int b = 1; b < NB; ++b) {
    Gx[b] = M::T.px[b] * cs[M::T.parent[b]] + M::T.pz[b] * sn[M::T.parent[b]];
    Gz[b] = M::T.pz[b] * cs[M::T.parent[b]] - M::T.px[b] * sn[M::T.parent[b]];
  }
  // hinges: height and velocity (root -> leaves)
  double Pz[NB], Vx[NB], Vz[NB];
  Pz[0] = q[1] + M::T.z0;
  Vx[0] = v[0];
  Vz[0] = v[1];
#pragma unroll
  for (int b = 1; b < NB; ++b) {
    Pz[b] = Pz[M::T.parent[b]] + Gz[b];
    Vx[b] = Vx[M::T.parent[b]] + om[M::T.parent[b]] * Gz[b];
    Vz[b] = Vz[M::T.parent[b]] - om[M::T.parent[b]] * Gx[b];
  }
  // ground contact: per body the force sum and its moment about the body's hinge
  double Fx[NB], Fz[NB], N[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    Fx[b] = 0.0;
    Fz[b] = 0.0;
    N[b] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < NSPH; ++k) {
    const int b = M::T.sbody[k];
    const double ox = M::T.su[k] * cs[b] + M::T.sw[k] * sn[b];
    const double oz = (M::T.sw[k] * cs[b] - M::T.su[k] * sn[b]) - M::T.srad[k];
    const double pen = -(Pz[b] + oz);
    const double vx = Vx[b] + om[b] * oz;
    const double vz = Vz[b] - om[b] * ox;
    const double fnr = HP_KC * pen - HP_CC * vz;
    const double fn = pen > 0.0 ? (fnr > 0.0 ? fnr : 0.0) : 0.0;
    const double lim = M::T.smu[k] * fn;
    const double fv = HP_CF * vx;
    const double fl = fv > -lim ? fv : -lim;
    const double ft = -(fl < lim ? fl : lim);
    Fx[b] = Fx[b] + ft;
    Fz[b] = Fz[b] + fn;
    N[b] = N[b] + (oz * ft - ox * fn);
  }
  // absolute-angle generalised forces: contact + gravity, the subtrees' contact forces on
  // their ancestors (children before parents)
  double w2[NB], Qa[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    w2[b] = om[b] * om[b];
    Qa[b] = N[b] + HP_GRAV * Sx[b];
  }
#pragma unroll
  for (int b = NB - 1; b > 0; --b) {
    const int a = M::T.parent[b];
    Qa[a] = Qa[a] + (Gz[b] * Fx[b] - Gx[b] * Fz[b]);
    Fx[a] = Fx[a] + Fx[b];
    Fz[a] = Fz[a] + Fz[b];
  }
  // the inertia in the absolute angles (only a body and its ancestors couple) and the
  // velocity terms
  double U[NB][NB], ca[NB];
#pragma unroll
  for (int a = 0; a < NB; ++a) {
    ca[a] = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) U[a][b] = a == b ? M::T.jc[a] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < NPAIRS; ++k) {
    const int a = M::T.pa[k], d = M::T.pd[k], c = M::T.pc[k];
    const double X = Gx[c] * Sx[d] + Gz[c] * Sz[d];
    const double Y = Gz[c] * Sx[d] - Gx[c] * Sz[d];
    U[a][d] = X;
    U[d][a] = X;
    ca[d] = ca[d] + w2[a] * Y;
    ca[a] = ca[a] - w2[d] * Y;
  }
  double cx = 0.0, cz = 0.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    cx = cx - w2[b] * Sx[b];
    cz = cz - w2[b] * Sz[b];
  }
  const double rx = Fx[0] - cx;
  const double rz = (Fz[0] - cz) - M::T.mt * HP_GRAV;
  // sums over subtrees: forces, S, and the inertia's columns, then its rows
  double Qs[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) Qs[b] = Qa[b] - ca[b];
#pragma unroll
  for (int b = NB - 1; b > 0; --b) {
    const int a = M::T.parent[b];
    Qs[a] = Qs[a] + Qs[b];
    Sx[a] = Sx[a] + Sx[b];
    Sz[a] = Sz[a] + Sz[b];
#pragma unroll
    for (int j = 0; j < NB; ++j) U[j][a] = U[j][a] + U[j][b];
  }
#pragma unroll
  for (int b = NB - 1; b > 0; --b) {
    const int a = M::T.parent[b];
#pragma unroll
    for (int j = 0; j < NB; ++j) U[a][j] = U[a][j] + U[b][j];
  }
  // joint coordinates: right-hand sides with the hinge forces, C's lower triangle with the
  // armature, the coupling rows
  double r[NB], B0[NB], B1[NB];
  r[0] = Qs[0];
#pragma unroll
  for (int b = 1; b < NB; ++b) {
    const int j = 2 + b;
    const double cv = CH_CH * v[j];
    const double flo = CH_KH * (M::T.lo[b] - q[j]) - cv, fhi = CH_KH * (M::T.hi[b] - q[j]) - cv;
    const double lim = q[j] < M::T.lo[b] ? flo : (q[j] > M::T.hi[b] ? fhi : 0.0);
    r[b] = M::T.sgn[b] * Qs[b] + (((tau[b - 1] - M::T.stiff[b] * q[j]) - M::T.damp[b] * v[j]) + lim);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    B0[b] = M::T.sgn[b] * Sz[b];
    B1[b] = -(M::T.sgn[b] * Sx[b]);
  }
  // Schur complement of the translational block, LDL^T in place: K's strict lower triangle
  // becomes L, d the pivots
  constexpr double imt = 1.0 / M::T.mt;
  double K[NB][NB], d[NB];
#pragma unroll
  for (int a = 0; a < NB; ++a) {
#pragma unroll
    for (int b = a; b < NB; ++b) {
      double cab = (M::T.sgn[a] * M::T.sgn[b]) * U[a][b];
      if (a == b) cab = cab + M::T.arm[a];
      K[b][a] = cab - (B0[a] * B0[b] + B1[a] * B1[b]) * imt;
    }
    r[a] = r[a] - (B0[a] * rx + B1[a] * rz) * imt;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    double dj = K[j][j];
#pragma unroll
    for (int c = 0; c < j; ++c) dj = dj - K[j][c] * K[j][c] * d[c];
    d[j] = dj;
#pragma unroll
    for (int i = j + 1; i < NB; ++i) {
      double val = K[i][j];
#pragma unroll
      for (int c = 0; c < j; ++c) val = val - K[i][c] * K[j][c] * d[c];
      K[i][j] = val / dj;
    }
  }
#pragma unroll
  for (int i = 1; i < NB; ++i)
#pragma unroll
    for (int c = 0; c < i; ++c) r[i] = r[i] - K[i][c] * r[c];
#pragma unroll
  for (int i = NB - 1; i >= 0; --i) {
    double val = r[i] / d[i];
#pragma unroll
    for (int c = i + 1; c < NB; ++c) val = val - K[c][i] * r[c];
    r[i] = val;
  }
  double tx = rx, tz = rz;
#pragma unroll
  for (int a = 0; a < NB; ++a) {
    tx = tx - B0[a] * r[a];
    tz = tz - B1[a] * r[a];
  }
  double qdd[NQ];
  qdd[0] = tx * imt;
  qdd[1] = tz * imt;
#pragma unroll
  for (int a = 0; a < NB; ++a) qdd[2 + a] = r[a];
#pragma unroll
  for (int i = 0; i < NQ; ++i) v[i] = v[i] + M::T.dt * qdd[i];
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = q[i] + M::T.dt * v[i];
}

// ------------------------------------------------------------------ HalfCheetah-v2: the env
__device__ inline void halfcheetah_reset(const double* u, double* s) {
  for (int i = 0; i < HC_NQ; ++i) s[i] = u[i] * 0.2 - 0.1;
  // Box-Muller of oracle/philox.py on the pairs (u10, u11) .. (u18, u19)
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double r = sqrt(-2.0 * log(1.0 - u[10 + 2 * k]));
    double sa, ca;
    sincos(2.0 * CH_PI * u[11 + 2 * k], &sa, &ca);
    s[HC_NQ + 2 * k] = 0.1 * (r * ca);
    if (2 * k + 1 < HC_NQ) s[HC_NQ + 2 * k + 1] = 0.1 * (r * sa);
  }
}

__device__ inline void halfcheetah_step(double* s, const float* a, double& rew, bool& done) {
  double tau[HC_ACT];
  double asq = 0.0;
#pragma unroll
  for (int k = 0; k < HC_ACT; ++k) {
    const double ak = (double)a[k];
    tau[k] = HcModel::T.gear[k + 1] * ch_clamp(ak, -HC_CTRL, HC_CTRL);
    asq = k == 0 ? ak * ak : asq + ak * ak;
  }
  const double xb = s[0];
#pragma unroll 1
  for (int f = 0; f < HC_NSUB; ++f) tree_substep<HcModel>(s, s + HC_NQ, tau);
  rew = (s[0] - xb) / HC_STEP - 0.1 * asq;
  done = false;
}

__device__ inline void halfcheetah_obs(const double* s, double* o) {
  for (int i = 0; i < HC_OBS; ++i) o[i] = s[1 + i];
}

struct HalfCheetahEnv {
  static constexpr int NS = HC_NS, OBS = HC_OBS, ACT = HC_ACT, DISCRETE = 0, MAX_STEPS = HC_MAX_STEPS, NU = HC_NU;
  __device__ static void reset(const double* u, double* s) { halfcheetah_reset(u, s); }
  __device__ static void obs(const double* s, double* o) { halfcheetah_obs(s, o); }
  __device__ static void step(double* s, const float* a, double& rew, bool& done) { halfcheetah_step(s, a, rew, done); }
};

}  // namespace mrl
