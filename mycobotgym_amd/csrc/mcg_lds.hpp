// mcg_lds.hpp -- the LDS slot map of the step kernels: every slot constant of the Reach and PickAndPlace columns, who owns a slot, who
// borrows it and until when.  A lane's column is an array of slots (slot k of a lane lives at base[k * STRIDE]: LaneScratchT in
// mcg_dynamics.hpp); the numbers below are slot indices.  An owned region is a row of a table that a static_assert tiles; a borrowed
// range has one static_assert that it lies inside its owner and, next to it, the sentence on why the two uses never meet (lifetimes are
// reasons, not types).  Included by mcg_dynamics.hpp, which defines `real`, NB and MCG_DEV first.
#pragma once

namespace mcg {

struct Span { int first, count; constexpr int end() const { return first + count; } };
constexpr bool inside(Span a, Span owner) { return a.count > 0 && a.first >= owner.first && a.end() <= owner.end(); }
template <int N> constexpr bool tiles(const Span (&parts)[N], Span whole) {       // in address order, no gap, no overlap
  int at = whole.first;
  for (int i = 0; i < N; i++) { if (parts[i].first != at || parts[i].count <= 0) return false; at = parts[i].end(); }
  return at == whole.end();
}

// =========================================================================================================== the Reach column (64 lanes)
// Per-lane scratch in LDS: slot k of this lane lives at base[k * 64] (lane-contiguous rows: conflict-free
// ds_read_b64 / ds_write_b64 with immediate offsets).  The joint-space inertia M is kept here between the stages
// that consume it, so that only one 12x12 system occupies registers at a time.
constexpr int LDS_M = 0;                              // packed lower triangle of M                     (78 slots)
constexpr int LDS_HEQ = NB * (NB + 1) / 2;            // H_eq = M + J^T D J over the equality (and weld) rows  (78 slots)
constexpr int LDS_SLOTS = 2 * (NB * (NB + 1) / 2);
// three-wave Reach kernel (SplitMainLocal / helper_substep): factor of M + hB, its reciprocal pivots, and q, qd published for the side waves
constexpr int LDS_FAC = LDS_SLOTS, LDS_FDINV = LDS_FAC + NB * (NB + 1) / 2, LDS_QB = LDS_FDINV + NB, LDS_QDB = LDS_QB + NB;
constexpr int LDS_FS = LDS_QDB + NB, LDS_WARM = LDS_FS + NB, LDS_QLAG = LDS_WARM + NB, LDS_IKT = LDS_QLAG + 6;      // LDS_WARM: qacc_warmstart parked between sub-steps; LDS_QLAG: q of the last forward pass; LDS_IKT: the IK controller's six ctrl increments of a control step, handed from the RNE wave to the main wave (two slots spare)
// The hand-over of the remote solve (SplitMainCols: the RNE wave solves the equality rows' system).  In EVERY sub-step the main wave
// parks its eight actuation forces (RACT: dofs 0..5, 6, 8 -- the other four are exactly zero) as soon as it has them and the constraint
// part of g0 (RG0, 12) likewise, and reads them back after S2 if it solves itself: neither stays in registers across the rows and the
// assembly of H_eq.  In a remote sub-step the RNE wave leaves abar in RA (12) before S3; the main wave prepares what the limit
// rows 6 and 8 need of its own numbers before S3 (gear_rows_prepare) and finishes the gear rows itself.  Lifetimes of the slots borrowed:
//   RA in WARM:       only the general iteration reads the warm start, a remote sub-step never runs it, and the Euler step after S3 writes
//                     the slots again (with a: from what the RNE wave left there, or zero in a lane that was reset) before the next
//                     sub-step could fall back and read them;
//   RACT = IKT:       the IK increments are live between the control-step barriers C1 and C2 only, the sub-steps run after C2;
//   RG0:              slots of its own.
constexpr int LDS_RA = LDS_WARM, LDS_RACT = LDS_IKT, LDS_RG0 = LDS_IKT + 8, LDS_SLOTS_SPLIT = LDS_RG0 + NB;
static_assert(LDS_RA + NB == LDS_QLAG && LDS_RACT >= LDS_QLAG + 6 && LDS_RACT + 8 <= LDS_RG0,
              "the remote solve's hand-over must stay inside the warm-start and IK-increment slots (the lagged q between them is live)");
static_assert(LDS_SLOTS_SPLIT * 64 * sizeof(real) <= 160 * 1024, "the split Reach kernel's LDS exceeds the 160 KB of a gfx950 workgroup");
// The sines and cosines of a sub-step, each evaluated by one of the three waves (trig_exchange), are exchanged between S1 and S1t in the
// FACTOR slots: the main wave's last read of the factor (after S3) comes before it reaches the next S1, and the helper's next write comes
// after the next S2, by which every wave has read its sines and cosines -- the two uses never overlap.
constexpr int LDS_SN = LDS_FAC, LDS_CS = LDS_SN + NB;
static_assert(LDS_SN >= LDS_FAC && LDS_CS + NB <= LDS_FDINV + NB && LDS_FDINV + NB == LDS_QB, "the sine / cosine exchange must lie inside the factor slots");
// The gear rows' columns z6 = H^-1 e_6, z8 = H^-1 e_8 (SplitMainCols::cols: the helper wave solves them between S2 and S3, the main
// wave reads them after S3).  Under that policy the main wave factors M + hB itself and nobody writes the factor slots, so the columns
// take 24 of them, behind the sine / cosine exchange: written after S2 and read before the next S1, they never meet it either.
constexpr int LDS_Z6 = LDS_CS + NB, LDS_Z8 = LDS_Z6 + NB;
static_assert(LDS_Z6 == LDS_FAC + 24 && LDS_Z6 >= LDS_SN + NB && LDS_Z6 >= LDS_CS + NB && LDS_Z8 == LDS_Z6 + NB && LDS_Z8 + NB <= LDS_QB,
              "the gear rows' columns must lie inside the factor slots, clear of the sine / cosine exchange and of the published q");
// What the main wave reads and writes around S3 under SplitMainCols -- the columns (Z6, Z8), abar and the warm start (RA = WARM), the
// published and the lagged state (QB, QDB, QLAG) -- lies within 128 slots, the reach of a ds_ offset field, but beyond it from slot 0:
// the main wave addresses these through a window of the lane's column that starts at LDS_WIN (LaneScratchT::window).
constexpr int LDS_WIN = LDS_QLAG + 6 - 128;
static_assert(LDS_WIN >= 0 && LDS_WIN <= LDS_Z6 && LDS_WIN <= LDS_QB && LDS_QDB + NB <= LDS_WIN + 128 && LDS_RA + NB <= LDS_WIN + 128
              && LDS_QLAG + 6 <= LDS_WIN + 128 && (128 - 1) * 64 * sizeof(double) < 65536,
              "the slots of the main wave's window must lie within one 16-bit ds_ offset of its base");
// The side waves' windows under SplitMainCols (WindowedScratchT in mcg_dynamics.hpp).  A single ds_ access reaches 128 slots from its
// base, the st64 pair form 256; a slot is served by the window whose single reach it lies in, so that no access needs an address op:
//   LDS_WIN_LO  the upper rows of H_eq (slots from 128 on) and the gear rows' columns; the sine / cosine exchange lies in its reach too.
//               Used by the helper wave (build_H, its stores of Z6 / Z8) and by the RNE wave (build_H of the remote solve);
//   LDS_WIN_HI  the published state, the bias forces and the remote solve's hand-over (QB, QDB, FS, RA, RACT, RG0).  Used by the RNE
//               wave: qd, no_other_rows and its store of passive - bias before S2, the remote solve after it.
// The exchange itself (trig_exchange, side_trig) is addressed from slot 0 in every wave: through these windows it was slower on either
// side wave and no faster on the main wave.
// Slots below LDS_WIN_LO are addressed from slot 0 as before; slots from LDS_WIN_SPLIT on go through the upper window, so that each
// region is served by one base as a whole and its neighbours pair.
constexpr int LDS_WIN_LO = 128, LDS_WIN_HI = LDS_SLOTS_SPLIT - 128, LDS_WIN_SPLIT = LDS_QB;
static_assert(LDS_WIN_LO <= 128 && LDS_WIN_LO > LDS_HEQ && LDS_WIN_LO <= LDS_SN && LDS_CS + NB <= LDS_WIN_LO + 128
              && LDS_Z8 + NB <= LDS_WIN_SPLIT && LDS_WIN_SPLIT <= LDS_WIN_LO + 128,
              "the lower side-wave window: slots below it within a ds_ offset of slot 0; H_eq's upper rows, the exchange and the columns, "
              "as every slot below the split, within one of its base");
static_assert(LDS_WIN_HI >= LDS_WIN_LO && LDS_WIN_HI <= LDS_WIN_SPLIT && LDS_WIN_SPLIT <= LDS_QB && LDS_QDB + NB <= LDS_WIN_HI + 128 && LDS_FS + NB <= LDS_WIN_HI + 128
              && LDS_RA + NB <= LDS_WIN_HI + 128 && LDS_RACT + 8 <= LDS_WIN_HI + 128 && LDS_RG0 + NB <= LDS_WIN_HI + 128,
              "the upper side-wave window: the published state, the bias forces and the remote solve's hand-over within one ds_ offset of its base");

// ==================================================================================================== the PickAndPlace column (32 lanes)
constexpr int PNP_LANES = 32;        // envs per wave in the PickAndPlace kernels: twice the LDS per env; a wave costs the
                                     // same with 32 or 64 active lanes (measured), and 8192 envs then cover all 256 CUs
constexpr int MAXCON = 16;           // list ENTRIES kept per env (a mesh's twin geoms: one entry of double weight); the oracle cuts its list at the
                                     // same entry (mco_model.maxentry).  MuJoCo has no cap; mcg_counters.contacts_dropped counts what this one cuts
constexpr int CON_STRIDE = 10;       // pos[3] n[3] dist D kterm type   (the tangents are re-derived from n: make_frame)
constexpr int ROW_SLOTS = 144;       // the row area: line-search rows of the cube-alone solve, cooperative workspaces, parked inputs
constexpr int NJW = 12;              // joints whose world axis + anchor are kept for the contact rows: all twelve
constexpr int WJ_STRIDE = 6, WJ_AXIS = 0, WJ_ANCHOR = 3;      // a joint's record in LDS_WJ: world axis 3, anchor 3

// ---- the owned regions, in address order: 640 slots x 32 lanes x 8 B, exactly the CU's 160 KB
constexpr int LDS_CON = 156;         // the contact list: CON_STRIDE slots per entry
constexpr int LDS_POLY = 316;        // 32 slots: the collision pass's two clip polygons, before barrier S2; afterwards the flags and the cube's hand-over (XCH_FLAG ..)
constexpr int XCH_Q = 348;           // 32 slots no pass writes, the robot side's exchange: q(t), qd(t), the hand-out counter, the carried active set
constexpr int LDS_ROW = 380;         // the row area (ROW_SLOTS): per pyramid row r0, dr of the cube-alone solve's line search; borrowed: see below
constexpr int LDS_ACT = 524;         // per contact: active-row bit mask of the cube-alone solve (as a double)
constexpr int LDS_WJ = 540;          // world axis + anchor of the twelve joints (WJ_STRIDE each)
constexpr int XCH_FS = 612;          // the robot's bias forces, RNE wave -> robot wave (SplitPnp::FS)
constexpr int MP_CUBE = 624;         // twelve slots of the mesh phase (mcg_mesh.hpp): MP_CUBE .. MP_DROP
constexpr int PUB_AREF_B = 636;      // aref of the limit rows 6..9, parked for the cooperative solve (the other six: PUB_AREF_A)
constexpr int PNP_SLOTS_LDS = 640;
constexpr Span RGN_M{LDS_M, NB * (NB + 1) / 2}, RGN_HEQ{LDS_HEQ, NB * (NB + 1) / 2}, RGN_CON{LDS_CON, MAXCON * CON_STRIDE}, RGN_POLY{LDS_POLY, 32},
               RGN_XCH{XCH_Q, 32}, RGN_ROW{LDS_ROW, ROW_SLOTS}, RGN_ACT{LDS_ACT, MAXCON}, RGN_WJ{LDS_WJ, WJ_STRIDE * NJW}, RGN_FS{XCH_FS, NB},
               RGN_MP{MP_CUBE, 12}, RGN_AREF_B{PUB_AREF_B, 4};
constexpr Span PNP_REGIONS[] = {RGN_M, RGN_HEQ, RGN_CON, RGN_POLY, RGN_XCH, RGN_ROW, RGN_ACT, RGN_WJ, RGN_FS, RGN_MP, RGN_AREF_B};
static_assert(tiles(PNP_REGIONS, Span{0, PNP_SLOTS_LDS}), "the owned regions must tile the PickAndPlace column without gap or overlap");
static_assert(PNP_SLOTS_LDS * PNP_LANES * sizeof(real) == 160 * 1024, "the PickAndPlace column is the 160 KB of a gfx950 workgroup, no more and no less");

// ---- RGN_POLY.  Before barrier S2 the collision pass clips there: two polygons of 8 vertices x 2 (a quadrilateral clipped by four
// half-planes has at most 8 vertices), source and destination swapping per half-plane.
constexpr int LDS_POLY_P = LDS_POLY, LDS_POLY_T = LDS_POLY + 16;
static_assert(tiles({Span{LDS_POLY_P, 2 * 8}, Span{LDS_POLY_T, 2 * 8}}, RGN_POLY), "the two clip polygons are the clip-polygon slots");
// After the collision pass (the clipping is over): flags and the cube's hand-over between the cube wave and the others.
// XCH_FLAG: 0 = no contact reaches the robot | 2 = one does (a pad or a mesh on the cube, the table or the ground), or the cube alone
// holds more contacts than its own solve has row slots for: the environment's 18 dofs go to the cooperative solve; bit 3: the cube failed
// mj_checkPos / mj_checkVel / mj_checkAcc (cube wave -> robot wave, read after S4).  XCH_T0: both pads touch the cube (cube wave ->
// robot wave, at the end of the env-step).  XCH_T1: the robot failed those checks (robot wave -> cube wave, read after S1);
// mj_resetData resets both bodies.
constexpr int XCH_FLAG = LDS_POLY, XCH_T0 = LDS_POLY + 1, XCH_T1 = LDS_POLY + 2, XCH_NCON = LDS_POLY + 3;
constexpr int XCH_CB = LDS_POLY + 4, XCH_QL7 = LDS_POLY + 23, XCH_DR = LDS_POLY + 30;      // cube: pos 3, quat 4, vel 6, warm 6; lagged pose 7; DR scales 2
constexpr int XCH_CB_POS = XCH_CB, XCH_CB_QUAT = XCH_CB + 3, XCH_CB_VEL = XCH_CB + 7, XCH_CB_WARM = XCH_CB + 13;      // the record of cube_to_lds / cube_from_lds (struct Cube)
static_assert(tiles({Span{XCH_FLAG, 1}, Span{XCH_T0, 1}, Span{XCH_T1, 1}, Span{XCH_NCON, 1}, Span{XCH_CB_POS, 3}, Span{XCH_CB_QUAT, 4},
                     Span{XCH_CB_VEL, 6}, Span{XCH_CB_WARM, 6}, Span{XCH_QL7, 7}, Span{XCH_DR, 2}}, RGN_POLY),
              "the flags and the cube's hand-over (its record ends where XCH_QL7 starts) are the clip-polygon slots");

// ---- RGN_XCH, which no pass writes: q(t), qd(t) of the robot for the other waves -- written at the end of a sub-step, read after
// S1 by the M, RNE and cube waves and between S4 and S5 by the cooperative solves -- and the workgroup's hand-out counter of that phase
// (an unsigned in the first word of lane 0's slot; coop_counter in mcg_coop.hpp).  XCH_SPARE: no code reads or writes it (the cube
// wave's verdict on the cube travels as bit 3 of XCH_FLAG, not in a slot of its own).
// XCH_ACT0 / XCH_ACT1: the active set the environment's last cooperative solve ended with, as raw bits -- [signature of the contact list |
// rows 0-31], [rows 32-63 | rows 64-95] -- cleared at the start of an env-step.  The next sub-step's solve starts from it (see coop_guess).
// XCH_CENSUS: the active set of two sub-steps ago, kept by -DMCG_STAGE_CLOCKS builds only (period-2 chatter census).
constexpr int XCH_QD = XCH_Q + NB, COOP_CTR_SLOT = XCH_QD + NB, XCH_SPARE = COOP_CTR_SLOT + 1;
constexpr int XCH_ACT0 = XCH_SPARE + 1, XCH_ACT1 = XCH_ACT0 + 1, XCH_CENSUS = XCH_Q + 30;
static_assert(tiles({Span{XCH_Q, NB}, Span{XCH_QD, NB}, Span{COOP_CTR_SLOT, 1}, Span{XCH_SPARE, 1}, Span{XCH_ACT0, 1}, Span{XCH_ACT1, 1},
                     Span{XCH_ACT1 + 1, 2} /* free */, Span{XCH_CENSUS, 2}}, RGN_XCH),
              "the robot side's exchange slots: state, counter word, carried active set, and the census in the last two");

// ---- RGN_ROW, borrowed three times over a sub-step:
//   between S1 and S1c: the frames of the bodies that carry candidate meshes (MP_FRAME, below);
//   after S2: the cube wave's own solves (ALONE_CON_SLOTS per contact -- six pyramid rows x (r0, dr) -- for list positions
//   0 .. ALONE_MAXCON - 1: a lane whose list is longer is flagged);
//   between barriers S4 and S5, when every lane-parallel solve is over: [0, COOP_WS_ROWS) cooperative workspace, COOP_WS_DOUBLES per wave.
constexpr int ALONE_CON_SLOTS = 12, ALONE_MAXCON = 12;
static_assert(inside(Span{LDS_ROW, ALONE_MAXCON * ALONE_CON_SLOTS}, RGN_ROW), "the cube-alone solve's line-search rows exceed the row area");
constexpr int COOP_WS_ROW = LDS_ROW, COOP_WS_ROWS = 96, COOP_WS_DOUBLES = 768;
static_assert(inside(Span{COOP_WS_ROW, COOP_WS_ROWS}, RGN_ROW) && 4 * COOP_WS_DOUBLES <= COOP_WS_ROWS * PNP_LANES,
              "cooperative workspace exceeds the first 96 rows of the row area");
// What the mesh phase (mcg_mesh.hpp) reads, columns of every lane.  MP_FRAME: the row area, free between barriers S1 and S2 (its solves run
// after S2): the world frame (rotation 9, origin 3) of each of the twelve robot bodies that carries a candidate mesh, parked by the wave
// whose broad phase found it -- ONE producer per body (M wave: bodies 0-3, RNE wave: 4, 5, cube wave: 6-11), so that a frame is one
// wave's arithmetic.
constexpr int MP_FRAME = LDS_ROW, MP_FRAME_STRIDE = 12, MP_FRAME_ROT = 0, MP_FRAME_POS = 9;
static_assert(inside(Span{MP_FRAME, MP_FRAME_STRIDE * NB}, RGN_ROW), "frames of the twelve bodies");

// ---- RGN_MP: twelve slots of the mesh phase's own.
constexpr int MP_CUBE_POS = MP_CUBE;                             // the cube's position (published when a sub-step ENDS: the M / RNE waves' broad phase reads it before S1b)
constexpr int MP_CUBE_QUAT = MP_CUBE + 3;                        // its normalised quaternion (written after S1, read in the mesh phase)
constexpr int MP_MASK = MP_CUBE + 7;                             // candidate pairs of the broad phases (bit 3 m + o; o: ground, table, cube), one slot per producer:
constexpr int MP_MASK_M = MP_MASK, MP_MASK_RNE = MP_MASK + 1, MP_MASK_CUBE = MP_MASK + 2;      // M wave, RNE wave, cube wave
constexpr int MP_NCON = MP_MASK + 3, MP_DROP = MP_NCON + 1;     // the list's length (the mesh phase appends); contacts the cap cut there
static_assert(tiles({Span{MP_CUBE_POS, 3}, Span{MP_CUBE_QUAT, 4}, Span{MP_MASK_M, 1}, Span{MP_MASK_RNE, 1}, Span{MP_MASK_CUBE, 1},
                     Span{MP_NCON, 1}, Span{MP_DROP, 1}}, RGN_MP), "the mesh phase's twelve slots");

// ---- the inputs of a lane's cooperative solve, parked by the robot wave (PubHook) -- right after S1b when the workgroup has a mesh phase to
// overlap with (then for every lane: the flags do not exist yet), else after S2 for the flagged lanes -- live in slots that are free from
// S1b to S5:
//   PUB_G0 in the robot's q(t) slots: read for the last time before S1b, rewritten when the sub-step ends;
constexpr int PUB_G0 = XCH_Q;
static_assert(inside(Span{PUB_G0, NB}, Span{XCH_Q, NB}), "g0 is parked in the robot's q(t) slots");
//   PUB_WARM, the warm start, in the bias-force slots: the robot wave has taken them; the RNE wave rewrites them after the next S1.  The
//   cooperative solve hands the robot's accelerations back there;
constexpr int PUB_WARM = XCH_FS;
static_assert(PUB_WARM == XCH_FS && RGN_FS.count == NB, "the warm start is parked in the bias-force slots");
//   PUB_SD, PUB_AREF_A, the limit rows, in the cube-alone solve's mask slots (a flagged lane has no such solve; an unflagged lane's solve
//   initialises its masks), and PUB_AREF_B: four slots of their own.
constexpr int PUB_SD = LDS_ACT, PUB_AREF_A = LDS_ACT + 10;
static_assert(inside(Span{PUB_SD, 10 + 6}, RGN_ACT) && PUB_AREF_A == PUB_SD + 10 && RGN_AREF_B.count == 10 - 6,
              "the limit rows borrow sixteen mask slots (ten sign * D, six aref) and own four");
MCG_DEV constexpr int pub_aref(int j) { return j < 6 ? PUB_AREF_A + j : PUB_AREF_B + (j - 6); }

}  // namespace mcg
