"""Every operator form the plan can select, per voxel, against the float64 reference of tests/ref64.py.

For each case a fresh child process (env switches are read once per process) builds the case's plan, reports the
form through ``plan.repeat_info`` (and, with UNIRES_SPLAT2_VERBOSE=1, which schedule build ran), and writes A p,
At v, AtA p, the matvec q with its float64 dot epilogue, and A / At / AtA of impulse combs to an .npz file.  The
parent checks every voxel against |out - ref| <= u c_M M + G + D (ref64) away from FOV ties, the float64 adjoint
identity and the dot against the same tolerances, and that the case ran on its form.  One child at a time, each
under a timeout; the first child that fails or dies ends the test; no retries.

Impulse combs put deltas (random values) at the volume's corners, at the first and last voxel of each axis' last,
partial tile (k_splat2 / k_ata1 tiles: 8 x 4 x 30) and of its first tile, and in the middle - in two combs, so
that the deltas of one comb lie further apart than the operator's footprint (2 (3 r + 4) + 1 voxels along an axis
of ratio r in y space, 8 voxels in x space) and each column / row is seen on its own.  In y space they give the
columns of A and AtA, in x space (the x volume's corners, ends and middle) the rows of A, through At.  They are
compared against the reference built with the taps the plan uses (``trimmed=True``), so D = 0 and a forward and an
adjoint that disagree on a tap or on the footprint show.

Case table (repeat_info: pull2 / splat2_axis / shift / fused / separable).  Where repeat_info cannot tell forms
apart, the kernels the env switch selects are named; the case then checks that the switch took effect where
repeat_info can show it, and relies on the switch otherwise:

| case               | geometry                                        | env                | form                                |
|--------------------|-------------------------------------------------|--------------------|-------------------------------------|
| z_thick            | 97x90x121, thick 6 along z, rot 0.12, scl 0.1   |                    | pull2 + splat2 AXIS 2               |
| z_thick_conc3      | the same, after plan.set_concurrency(3)         |                    | pull2 + splat2 AXIS 2               |
| x_thick, y_thick   | 41x38x61, thick 4 along x / y                   |                    | pull2 + AXIS 0 / AXIS 1             |
| iso2_rect          | 42x38x61 (x-space z 30), ratio 2, scl 0.1       |                    | hybrid: pull2 + AXIS 2, not sep.    |
| iso2_rect_z4       | 42x38x64 (x-space z 32, a multiple of 4)        |                    | hybrid: pull2 + AXIS 2, not sep.    |
| iso2_rect_nohyb    | 42x38x61, scl 0 (AXIS 3 scales along z only)    | UNIRES_NO_HYBRID=1 | splat2 AXIS 3                       |
| iso2_gauss         | 34x30x36, ratio 2, Gaussian in-plane            |                    | separable passes; dropped taps      |
| denoise            | 41x38x61, rot 0.1                               |                    | k_ata1 (fused)                      |
| denoise_noata1     | the same                                        | UNIRES_NO_ATA1=1   | pull2 + splat2 AXIS -1              |
| translate          | 41x38x60, thick 6 along z, fractional shift     |                    | shift kernel (matvec)               |
| translate_noshift  | the same                                        | UNIRES_NO_SHIFT=1  | two-kernel matvec                   |
| int_shift          | 41x38x61, thick 6 along z, shift (2, -1, 3)     |                    | k_ata_aligned* (matvec; the shift   |
|                    |                                                 |                    | kernel declines: z not 4k)          |
| int_shift_noalign  | the same                                        | UNIRES_NO_ALIGNED=1| two-kernel matvec                   |
| int_shift_z60      | 41x38x60, thick 6 along z, shift (2, -1, 3)     |                    | k_ata_aligned*, 16-byte form (z 4k; |
|                    |                                                 |                    | the shift tables exist too)         |
| identity           | 37x41x53 (not a multiple of the 2048 chunk)     |                    | k_dtd_flat (regime id)              |
| identity_noflat    | the same                                        | UNIRES_NO_FLAT=1   | the line stencil kernel             |
| orient_9 / _22     | 41x38x61, thick 4, stored as SIGNED_PERMS 9/22  |                    | canonicalised, pull2 + splat2       |
| z_nosplat2         | 41x38x61, thick 6 along z, rot 0.1, scl 0.1     | UNIRES_NO_SPLAT2=1 | k_splat (no schedule)               |
| z_pushtile         | the same                                        | UNIRES_PUSH=tile   | k_push_tile (the schedule is built, |
|                    |                                                 |                    | the switch bypasses it: not visible)|
| z_nopull2          | the same                                        | UNIRES_NO_PULL2=1  | k_pull_conv on R.Af / R.Tf          |
| dn_nopull2         | denoise                                         | NO_PULL2, NO_ATA1  | k_pull + splat2 AXIS -1             |
| ctab_1266 / _1272  | 24x20x1266 / 1272, thick 6 along z: conv table  |                    | AXIS 2 / no schedule                |
|                    | of 1267 / 1273 entries (limit gn + 128 <= 1400) |                    |                                     |
| rowcode_724 / _725 | 724x724x12 / 725x724x12, thick 6 along z:       |                    | AXIS 2 / no schedule                |
|                    | gd.x rows_y = 524176 / 524900 against 2^19 - 1  |                    |                                     |
| ax0_gdy511 / _512  | 24x511x20 / 24x512x20, thick 4 along x          |                    | AXIS 0 / no schedule (gd.y <= 511)  |
| ax1_gdy509 / _513  | 24x508x20 / 24x512x20, thick 4 along y: gd.y    |                    | AXIS 1 / no schedule                |
|                    | 509 / 513 (4 n + 1: 511 and 512 are not grids)  |                    |                                     |
| sweep_*            | z-thick (thick 6, 41x38x61) and denoise, at     |                    | SWEEP_FORMS: two-pass schedule      |
|                    | 0.3 / 0.5 / 0.7 / 0.78 rad about x and about y  |                    | build (staging-slot overflow) at    |
|                    |                                                 |                    | 0.3 / 0.5; no splat2 / k_ata1 at    |
|                    |                                                 |                    | 0.7; no pull2 at 0.78 about x       |

The conv-table pair: a rect profile at ratio r has r + 1 taps, so the table has r n_x + 1 entries: 1272 itself is
no table length at ratio 6, and 1267 / 1273 are the two lengths either side of the limit.

The last-resort forward (api_operator.hip: forward, launch_pull + conv_down on the untrimmed R.A /
R.T / R.dim_g) runs only when launch_pull_conv fails.  launch_pull_conv (fused.hip) halves its output tile
(pick_out_tile) down to one voxel until the pulled tile fits 24 KB of LDS, so it fails (over 64 KB) only when the
product of the taps exceeds ~16k.  Such profiles are separable (R.sep: more than 64 taps in all) and run the
separable passes on R.Af / R.Tf; the hybrid form, which resets sep, is kept only where the window plan of pull2
exists (build_repeat_kernels) and its forward is the hybrid branch.  So that path is not reached, and its untrimmed taps
never meet the trimmed push.  z_nopull2 runs k_pull_conv, on the trimmed R.Af / R.Tf.

Observed on an MI355X (largest err / tol over every check of the case; voxels excluded as FOV ties): z_thick 0.350
/ 300, z_thick_conc3 0.350 / 300, x_thick 0.288 / 0, y_thick 0.296 / 0, iso2_rect 0.394 / 0, iso2_rect_z4 0.335 / 0,
iso2_rect_nohyb 0.394 / 0, iso2_gauss 1.000 / 0 (voxels only the dropped taps reach: the kernel returns 0, err = D),
denoise 0.400 / 0, denoise_noata1 0.400 / 0, translate 0.038 / 0, translate_noshift 0.035 / 0, int_shift 0.025 / 0,
int_shift_noalign 0.025 / 0, int_shift_z60 0.030 / 0, identity 0.151 / 0, identity_noflat 0.156 / 0, orient_9 0.141
/ 0, orient_22 0.158 / 0,
z_nosplat2, z_pushtile, z_nopull2 0.257 / 0, dn_nopull2 0.400 / 0, ctab_1266 0.403 / 2144, ctab_1272 0.229 / 3187,
rowcode_724 0.284 / 22442 (of 6.3M), rowcode_725 0.271 / 24686, ax0_gdy511 0.237 / 662, ax0_gdy512 0.247 / 602,
ax1_gdy509 0.237 / 386, ax1_gdy513 0.374 / 657, the sweep 0.111 - 0.376 / 0; the 256^3 matvec 0.156 / 3302.  The
most instructions in one tile: 23 - 26 below 0.3 rad, 33 - 48 in the two-pass sweep cases.  No case failed: the
suite found no kernel bug.

The stride-2 conv passes across their block seams (``SEAM_CASES``; conv.hip).  With UNIRES_CONV_VERBOSE=1 the child
reports on stderr which kernel each separable pass launched ([conv] lines, one per instantiation); a case's ``conv``
entry names the kernels that must be among them, those that only A p on its own launches (the table with a non-forward
D does not run it) and those that must not: a miss is drift, like ``expect``.  The kernels work in blocks and runs,
read off conv.hip: k_conv_ydown_xdownup2<NY,NX,FX,FY> owns OWN = 32 x-space rows per y block (gy > 0, conv_up_y as
well: 32 - (FY - 1)), 8 float4 = 32 x-space z per z block, and marches along x in runs of >= 6 x-space steps;
k_conv_up_yz2 forms 32 grid rows per y block and takes x-space z <= 512; k_conv1d_up_z2 and k_conv_up_yz2 pass
along z 61 lane pairs = 244 grid z at a time, three halo lanes moved by DPP shifts; the marching passes
k_conv1d_down2_m / _up2_m / _downup2_m walk runs of 8 outputs / input steps; conv1d_grid gives the gather and z passes
at most 48 workgroups along x, which loop over the x slabs.  The smaller cases above stay inside the first block of each.
Here 26x70x72 (x space 13x35x36, grids 27 - 33 x 71 - 77 x 73 - 79) has two y blocks for every tap count, two z
blocks (9 float4), three x runs (14 - 17 steps of 6), three y blocks of k_conv_up_yz2 and more than 8 marching steps
along x and y; the long-z shapes cross the 244-voxel passes and stand either side of the 512 limit; 150x18x24 at
ratio 3 (x space 50x6x8, grid 152x30x36) has more x slabs than workgroups along x.  With all ratios equal the thick
axis is x: a Gaussian in-plane profile (prof_ip 2) lies along y and z, the through-plane profile (prof_tp; rect: 3
taps kept, triangle 5, Gaussian 9 of 11) along x.  Every case is thick 2, iso (2, 2, 2), rot 0.1, trans 1.0 unless
it says otherwise; the seeds are part of the cases (no voxel is excluded as a FOV tie with them, other seeds exclude
up to half a volume: tests/test_voxelwise_comparator.py holds each case to the cap on the CPU).

``tile``: where ``comb`` puts its deltas, per case the y-space images of the seams (x: 2 run, y: 2 OWN, z: 64 or
the 244-voxel pass; 16 = 2 x 8 for the marching runs; 144 = 3 x 48 for the x slabs).  At spacing 21 an axis of 26,
70 or 72 voxels holds two or three deltas: the combs of 26x70x72 land on x 0, 24 / 1, 25 (24: the second run's
first plane), y 0, 35, 64 / 1, 35, 69 and z 0, 36, 64 / 1, 36, 71 - the first voxel past each seam, whose column
reaches 10 voxels back across it; the long-z combs on z 0, 244, 516, 976, 1031 / 1, 243, 516, 975, 1031 (z 1032).
Ratio 3 with the 15-tap Gaussian has a footprint of 33 along y and z: ``spacing`` (27, 33, 33) there.

| case                  | kwargs (besides the above), seed, env      | seam it is there for; tile                | [conv] kernels observed on an MI355X                   |
|-----------------------|--------------------------------------------|-------------------------------------------|--------------------------------------------------------|
| sep2_gauss            | prof_ip 2, scl 0.05; seed 9                | k_conv_ydown_xdownup2, gy = 0: y, z       | k_conv_ydown_xdownup2<9,3,2,0>, k_conv_up_yz2<5>,      |
|                       |                                            | blocks, x runs; k_conv_up_yz2 y blocks;   | k_conv1d_up2_m<2>; A p: k_conv1d_down2_m<9>, <3>       |
|                       |                                            | (12, 64, 64)                              |                                                        |
| sep2_gauss_noyx       | the same; UNIRES_CONV_YX=0                 | k_conv1d_downup2_m: runs, warm-up steps;  | k_conv1d_down2_m<9>, k_conv1d_downup2_m<3,2>,          |
|                       |                                            | (16, 16, 64)                              | k_conv_up_yz2<5>, k_conv1d_up2_m<2>, ..down2_m<3>      |
| sep2_gauss_march      | the same; UNIRES_CONV_YX=0,                | the three marching passes on their own,   | k_conv1d_down2_m<9>, <3>, k_conv1d_up2_m<2>, <5>,      |
|                       | UNIRES_CONV_DOWNUP=0, UNIRES_UPYZ_LDS=0    | k_conv1d_up_z2; (16, 16, 64)              | k_conv1d_up_z2                                         |
| sep2_gauss_tri        | prof_ip 2, prof_tp 1; seed 9               | the 5-tap instantiations beside the       | k_conv_ydown_xdownup2<9,5,3,0>, k_conv_up_yz2<5>,      |
|                       |                                            | 9-tap ones; (12, 64, 64)                  | k_conv1d_up2_m<3>; A p: k_conv1d_down2_m<9>, <5>       |
| sep2_allgauss         | prof_ip 2, prof_tp 2, scl 0.05; seed 9     | 9 taps on every axis; (12, 64, 64)        | k_conv_ydown_xdownup2<9,9,5,0>, k_conv_up_yz2<5>,      |
|                       |                                            |                                           | k_conv1d_up2_m<5>; A p: k_conv1d_down2_m<9>            |
| sep2_allgauss_nopull2 | the same; UNIRES_NO_PULL2=1                | conv_down along z as a pass of its own;   | k_conv_up_yz2<5>, k_conv1d_up2_m<5>; A p and A^T A:    |
|                       |                                            | (16, 16, 64)                              | k_conv1d_down_z, k_conv1d_down2_m<9>                   |
| sep2_rect             | scl 0.1; seed 11                           | the hybrid `both` branch, gy > 0: OWN =   | k_conv_ydown_xdownup2<3,3,2,2>,                        |
|                       |                                            | 31, two y blocks; (12, 62, 64)            | k_conv2d_up_xy_v4_t<2,2,4>; A p: k_conv2d_down_xy_v4   |
| sep2_rect_noxy        | the same; UNIRES_CONV_YX=0,                | the 3-tap marching passes instead;        | k_conv1d_down2_m<3>, k_conv1d_up2_m<2>                 |
|                       | UNIRES_CONV_XY=0                           | (16, 16, 64)                              |                                                        |
| sep2_tri              | prof_ip 1, prof_tp 1; seed 11              | 5 taps on every axis; (12, 64, 64)        | k_conv_ydown_xdownup2<5,5,3,0>, k_conv_up_yz2<3>,      |
|                       |                                            |                                           | k_conv2d_up_xy_v4_t<3,3,2>, k_conv1d_up_z2; A p:       |
|                       |                                            |                                           | k_conv1d_down2_m<5>                                    |
| sep2_z256             | 24x20x256, prof_ip 2, prof_tp 2, angles    | k_conv1d_up_z2, grid z 263 > 244: a       | k_conv1d_up_z2, k_conv1d_up2_m<5>,                     |
|                       | (0, 0, 0.04); seed 3; UNIRES_UPYZ_LDS=0    | second pass, its halo; (8, 4, 244)        | k_conv_ydown_xdownup2<9,9,5,0>; A p: ..down2_m<9>      |
| sep2_z1024            | the same at 24x20x1024 (x-space z 512)     | k_conv_up_yz2 at the last z of its        | k_conv_up_yz2<5>, k_conv1d_up2_m<5>,                   |
|                       |                                            | domain, five passes; (8, 4, 244)          | k_conv_ydown_xdownup2<9,9,5,0>; A p: ..down2_m<9>      |
| sep2_z1032            | the same at 24x20x1032 (x-space z 516)     | past it: the two passes; (8, 4, 244)      | k_conv1d_up2_m<5>, k_conv1d_up_z2,                     |
|                       |                                            |                                           | k_conv_ydown_xdownup2<9,9,5,0>; A p: ..down2_m<9>      |
| sep3_x150             | 150x18x24, thick 3, iso (3, 3, 3), prof_ip | 50 / 152 x slabs on a grid.z of 48;       | k_conv1d_up<float4>, k_conv1d_up_z; A p and A^T A:     |
|                       | 2, rot 0.05; seed 1                        | (144, 6, 12)                              | k_conv1d_down<float4>                                  |
| sep3_x150_nopull2     | the same; UNIRES_NO_PULL2=1                | k_conv1d_down_z over 152 x slabs;         | the same and k_conv1d_down_z                           |
|                       |                                            | (144, 6, 12)                              |                                                        |

k_conv1d_down_z: a plan with profiles along x or y and along z takes conv_down along z into its window pull
(k_pull_conv2 on R.Tz, the hybrid and the forward-only hybrid forms of api_plan.hip), so no geometry of these reaches the z pass
while the window plan exists; it runs where pull2 declines (here: under UNIRES_NO_PULL2, which also
closes the one-kernel A^T A forms: they start from the window pull).  sep2_allgauss therefore does not run it, and
the two _nopull2 cases are there for it.

Observed on an MI355X (largest err / tol over every check of the case; no voxel excluded in any of them): sep2_gauss,
sep2_gauss_noyx, sep2_gauss_march 0.730 (A^T v; A^T A p 0.297 in all three), sep2_gauss_tri 0.683, sep2_allgauss
0.656, sep2_allgauss_nopull2 0.656, sep2_rect, sep2_rect_noxy 0.404, sep2_tri 0.378, sep2_z256 0.115, sep2_z1024
0.111, sep2_z1032 0.138, sep3_x150 0.203, sep3_x150_nopull2 0.203.  With a non-forward D: sep2_gauss q 0.026 / 0.050, b
0.391 / 0.412; sep2_rect q 0.076 / 0.153, b 0.391 / 0.391.  No case failed: no kernel is wrong across a seam.

The one-kernel matvec forms (``ONE_KERNEL_CASES``; shift.hip, aligned.hip).  Which instantiation holds the whole matvec
is decided by shape and alignment alone (launch_ata_shift, shift_nl, shift_xr, shift_fast, shift_build; launch_lines,
launch_ata_aligned, launch_dtd_lines) and repeat_info only says that the shift tables exist.  With
UNIRES_MATVEC_VERBOSE=1 the child reports on stderr every instantiation it launches ([matvec] lines: the name with its
template arguments - k_ata_shift_m<NL, DOT, OBJ, FAST>, k_ata_shift2 / k_ata_shift<DOT, OBJ>, k_ata_aligned<NP, DOT, OBJ>,
k_ata_aligned4<NP4, DOT, OBJ>, k_ata_aligned4x2<DOT, OBJ> - the grid, and the run-time facts that select code inside it); a
case's ``matvec`` entry names the form that must run, a condition on those facts, and for aligned.hip the caller; any
other one-kernel launch is drift, like ``expect``.  The one-kernel forms serve the matvec only (A p, A^T v and A^T A p of
proj_apply run the general kernels: the combs and the adjoint identity check those, on these geometries), so for
these cases the child also assembles b = plan.rhs and runs the two one-iteration solves of the non-forward table with
forward differences: the matvec with its dot is the <.., 1, 0> instantiation, entry 0 of a 'max_gain' solve comes from a
stored <.., 0, 0> matvec, entry 1 of a 'max_gain_fresh' solve is the <.., 1, 1> one (the data term read from registers,
nothing stored); both objectives are held to ``obj_check``'s bound with ref64's bound_matvec as the float64 side, and
all three instantiations must be among the [matvec] lines.  Every case: thick slices along z, no rotation, an exact
translation (make_problem(shift=): at thick 6 the first point of the trimmed grid the kernels run on lies at z =
shift_z - 3, and oz is its floor), seed 11, scl 0.1; comb tile (4, 2, 64): the x run, the pair of lines, the 4-voxel lane.  No voxel of any case is a FOV tie.

| case            | dim_y, thick, shift            | there for                              | [matvec] observed on an MI355X (the <.., 1, 0> line)           |
|-----------------|--------------------------------|----------------------------------------|----------------------------------------------------------------|
| tr_yodd         | 41x37x60, 6, (.3, -.6, .4)     | odd y: NL = 1 (shift_nl)               | k_ata_shift_m<1,1,0,0> grid 102 xr 4 lw 1 padl 4 padr 0 nf 8   |
| tr_yodd_z256    | 12x9x256, 6, (.3, -.6, 2.4)    | NL = 1, FAST (256-voxel lines)         | k_ata_shift_m<1,1,0,1> grid 7 xr 4 lw 1 padl 4 padr 0 nf 8     |
| int_yodd_z256   | 10x11x256, 6, (2, -1, 3)       | integer weights through it (tried      | k_ata_shift_m<1,1,0,1> grid 9 xr 4 lw 1 padl 0 padr 0 nf 8     |
|                 |                                | before the aligned kernel)             |                                                                |
| tr_thick2       | 20x18x40, 2, (.3, -.6, .4)     | stride 2, nf = 4; shift_build finds    | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 1 nf 4    |
|                 |                                | four-entry lane windows: lw 1          |                                                                |
| tr_thick3       | 20x18x48, 3, the same          | nf = 6 (five taps: see below)          | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 1 nf 6    |
| tr_thick4       | 20x18x48, 4, the same          | nf = 6                                 | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 0 nf 6    |
| tr_xdz128       | 12x10x256, 2, the same         | xd.z = 128 > 64: no lane window (lw    | k_ata_shift_m<2,1,0,0> grid 4 xr 4 lw 0 padl 4 padr 1 nf 4     |
|                 |                                | 0), zline_taps, its k0 loop twice      |                                                                |
| tr_zpos         | 20x18x60, 6, (.3, -.6, 9.6)    | right apron (oz 6, padr 8)             | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 0 padr 8 nf 8    |
| tr_zneg         | 20x18x60, 6, (.3, -.6, -7.4)   | left apron (oz -11), empty e / e4 rows | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 12 padr 0 nf 8   |
| tr_xyout        | 20x18x60, 6, (-3.3, 4.6, .4)   | masked rows of cx / cy, planes and     | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 0 nf 8    |
|                 |                                | lines wholly outside                   |                                                                |
| tr_z8           | 9x6x8, 2, (.3, -.6, .4)        | the shortest line, two live lanes      | k_ata_shift_m<2,1,0,0> grid 3 xr 4 lw 1 padl 4 padr 1 nf 4     |
| tr_x3           | 3x4x8, 2, the same             | dim_y.x < 4 <= xr: one run, both faces | k_ata_shift_m<2,1,0,0> grid 1 xr 4 lw 1 padl 4 padr 1 nf 4     |
| tr_z260         | 9x6x260, 6, the same           | just outside (z > 256): shift False    | none: the general pair                                         |
| tr_x1028        | 1028x6x8, 2, the same          | x > 1024 (shift_xr 0), even y          | k_ata_shift2<1,0> grid 1542 xr 0 lw 1 padl 4 padr 1 nf 4       |
| tr_x1028_yodd   | 1028x5x8, 2, the same          | the same, odd y                        | k_ata_shift<1,0> grid 1285 xr 0 lw 1 padl 4 padr 1 nf 4        |
| tr_tri4         | 20x18x48, 4, prof_tp 1, (.3,   | nine taps at stride 4: fan-in 3, which | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 2 nf 10   |
|                 | -.6, .4)                       | shift_build's triples hold             |                                                                |
| int_tri4        | the same, (2, -1, 3)           | launch_ata_aligned declines (fan-in >  | k_ata_shift_m<2,1,0,0> grid 12 xr 4 lw 1 padl 4 padr 5 nf 10   |
|                 |                                | 2); the shift kernel takes it          |                                                                |
| int_yodd_z60    | 41x37x60, 6, (2, -1, 3)        | 16-byte form, odd y                    | k_ata_aligned4<1,1,0> grid 380 ata padl 4 padr 1 nk 7 s 6      |
| int_z300        | 9x8x300, 6, the same           | two 256-voxel passes per line          | k_ata_aligned4<2,1,0> grid 18 ata padl 4 padr 1 nk 7 s 6       |
| int_z203 / _323 | 9x8x203 / 323 / 451, the same  | the dword form at 4 / 6 / 8 passes     | k_ata_aligned<4,1,0> / <6,1,0> / <8,1,0> grid 18 ata padl 1    |
| / _451          |                                |                                        | padr 1 nk 7 s 6                                                |
| int_z512 / _516 | 9x8x512 / 516, the same        | either side of the limit               | k_ata_aligned4<2,1,0> (as int_z300) / none: the general pair   |
| int_zneg        | 20x18x61, 6, (2, -1, -5)       | left apron (oz -8)                     | k_ata_aligned<2,1,0> grid 90 ata padl 8 padr 1 nk 7 s 6        |
| int_zpos        | 20x18x61, 6, (2, -1, 9)        | right apron (oz 6)                     | k_ata_aligned<2,1,0> grid 90 ata padl 1 padr 6 nk 7 s 6        |
| id_z203 / _323  | 9x8x203 / 323 / 451, A = I,    | the line stencil at npt 4 / 6 / 8      | k_ata_aligned<4,1,0> / <6,1,0> / <8,1,0> grid 18 dtd padl 1    |
| / _451          | UNIRES_NO_FLAT=1               |                                        | padr 1 nk 1 s 1                                                |
| id_z516         | 9x8x516, the same              | past launch_dtd_lines' 512             | none: k_dtd                                                    |

Each case with A != I also showed the <.., 0, 0> and <.., 1, 1> lines of the same instantiation with the same facts.
Expectations the code settled otherwise than first written down: tr_thick3 was put down for nf = 5, but a rect
profile's taps are symmetric about their centre and so odd in number - 3, 5, 5, 7 at ratio 2, 3, 4, 6 (trim_taps keeps all
of them) - so ratio 3 runs on five taps like ratio 4, nf = 6, and no rect profile gives nf = 5; the tap counts that are
no multiple of four are 6 and the triangle's 10.  tr_thick2 was expected on the per-voxel triples (stride below 4); shift_build
tests the windows themselves, and at stride 2 with three taps the four rows of every lane span at most four x-space
entries, so lw 1: the triple form (lw 0) is reached through xd.z > 64 alone (tr_xdz128).

Observed on an MI355X (largest err / tol over every check of the case; no voxel excluded in any): tr_yodd 0.028,
tr_yodd_z256 0.037, int_yodd_z256 0.030, tr_thick2 0.018, tr_thick3 0.024, tr_thick4 0.024, tr_xdz128 0.022, tr_zpos 0.035,
tr_zneg 0.044, tr_xyout 0.041, tr_z8 0.025, tr_x3 0.019, tr_z260 0.025, tr_x1028 0.027, tr_x1028_yodd 0.023, tr_tri4 0.022,
int_tri4 0.020, int_yodd_z60 0.024, int_z300 0.023, int_z203 0.018, int_z323 0.026, int_z451 0.031, int_z512 0.023, int_z516
0.025, int_zneg 0.028, int_zpos 0.029, id_z203 0.110, id_z323 0.148, id_z451 0.189, id_z516 0.138; the objectives at most
0.003 of their bound.  One kernel bug found and fixed: k_ata_aligned4<2> (int_z300, int_z512: q off by up to 1e4 times
its tolerance in the two voxels z = 255 and 256 of every line, 144 voxels a case).  Its lanes take the z neighbour across
the seam of the two 256-voxel passes from the other pass' register with __builtin_amdgcn_readlane; the builtin is
declared on int, so handed a float it returned the neighbour truncated to an integer, and the stencil's z differences
at the seam were off by the neighbour's fraction.  aligned.hip now passes the bits (a4_readlane).  The norm gates
could not see two voxels in 300.

The table with a non-forward D (``DIFF_CASES``, ``test_every_form_per_voxel_with_backward_and_central_differences``).
A plan with sett.diff = 'backward' / 'central' composes its matvec differently (api_operator.hip, matvec):
every AtA kernel runs without its stencil epilogue, and one pass - k_dtd_flat_w<W, ACC>, or k_dtd<W, ACC> where the
flat kernel declines the shape - adds c DtD_W p to the stored q and closes the matvec with the dot or the objective.
One child per case sets each difference in turn on the same plan and writes q with its float64 dot, the right-hand
side b (k_div<W>, then the accumulating A^T of every repeat) and the objectives of two one-iteration solves from
x0 = p; the parent checks q per voxel against ref64.bound_matvec_reps, the dot against the float64 dot of the stored
vectors, b per voxel against ref64.bound_rhs, and the objectives (``_check_diff``).  The cases are the forms above by
name (z_thick and z_thick_conc3 at 41x38x61; no table limits, no sweep: those exercise the schedule; of the seam cases
sep2_gauss and sep2_rect: without the stencil epilogue the accumulating stores behind their passes change) and:

| case               | geometry                                        | what it is there for                                |
|--------------------|-------------------------------------------------|-----------------------------------------------------|
| z_aniso, dn_aniso  | z_thick's / denoise's, voxels 0.8x1.25x2.0 mm   | cx != cy != cz in the closing pass                  |
| sr_2rep            | 41x38x61, thick 4, two repeats (thick z, y)     | accumulating stores, the stencil added once         |
| dn_2rep            | 21x19x33, denoising, two repeats                | the same on k_ata1                                  |
| dn_under64         | 3x2x5 (30 voxels)                               | k_dtd<W, ACC>: fewer than 64 voxels                 |
| dn_nz3             | 12x10x3                                         | k_dtd<W, ACC>: lines shorter than 4                 |
| translate_z256,    | 12x10x256 fractional shift, 10x12x256 shift     | the shift kernel's fast form (256-voxel lines       |
| int_shift_z256     | (2, -1, 3); thick 6 along z                     | only), tried first by a one-repeat plan             |
| z_unaligned,       | z_thick's / denoise's, out= a view 1, 2, 3      | head, the per-voxel tail and ld4_safe(rq) of the    |
| dn_unaligned       | floats into a sentinel-padded buffer            | ACC pass; pads unchanged, every voxel written       |
| tr_yodd, tr_x1028, | ONE_KERNEL_CASES' by name                       | the <.., 0, 0> instantiations of k_ata_shift_m<1>,  |
| tr_x1028_yodd,     |                                                 | k_ata_shift2, k_ata_shift, the triple form (lw 0),  |
| tr_xdz128, tr_zpos,|                                                 | a right apron, k_ata_aligned4<1>, <2> and           |
| int_yodd_z60,      |                                                 | k_ata_aligned<6>: zero stencil weights, no partials,|
| int_z300, int_z323 |                                                 | stencil_close behind them                           |
| translate_unaligned| translate's, out= as z_unaligned                | launch_ata_shift declines an unaligned q: the       |
|                    |                                                 | general pair, no [matvec] line before the solves    |
| int_z60_unaligned  | int_shift_z60's, out= as z_unaligned            | launch_lines leaves k_ata_aligned4x2 for the dword  |
|                    |                                                 | form k_ata_aligned<2,0,0>                           |

With a non-forward D every one-kernel launch must be a <.., 0, 0> instantiation (``matvec_drift``), the case's among them.
The two unaligned cases state the form of the matvecs into the unaligned ``out``; the child marks on stderr where its
first right-hand side and solve begin ([phase]), which run on aligned vectors of their own and so on the 16-byte
forms (observed: k_ata_shift_m<2,0,0,0> / k_ata_aligned4x2<0,0>, both only after the mark).

int_shift_z60 does not reach the shift kernel's fast form (shift_fast wants 256-voxel lines): at z = 60 an integer
shift runs aligned.hip's 16-byte form; the two z256 cases are there for that branch.

Observed on an MI355X (err / tol, backward / central; no voxel excluded in any case): the matvec q 0.047 / 0.091
(z_thick, z_thick_conc3, z_nosplat2, z_pushtile, z_nopull2, z_unaligned at all three offsets), 0.084 / 0.108 (x_thick),
0.066 / 0.129 (y_thick), 0.039 / 0.074 (iso2_rect), 0.039 / 0.065 (iso2_rect_nohyb), 0.014 / 0.025 (iso2_gauss),
0.170 / 0.258 (denoise, denoise_noata1, dn_nopull2, dn_unaligned), 0.038 / 0.033 (translate), 0.037 / 0.033
(translate_noshift), 0.024 / 0.025 (int_shift, int_shift_noalign), 0.029 / 0.029 (int_shift_z60), 0.114 / 0.123
(identity), 0.040 / 0.073 (orient_9), 0.083 / 0.089 (z_aniso), 0.094 / 0.134 (dn_aniso), 0.104 / 0.223 (sr_2rep),
0.119 / 0.176 (dn_2rep), 0.009 / 0.010 (dn_under64), 0.045 / 0.079 (dn_nz3), 0.031 / 0.024
(translate_z256), 0.024 / 0.024 (int_shift_z256), 0.028 / 0.023 (tr_yodd), 0.027 / 0.017 (tr_x1028), 0.020 / 0.015
(tr_x1028_yodd), 0.017 / 0.013 (tr_xdz128), 0.035 / 0.040 (tr_zpos), 0.024 / 0.026 (int_yodd_z60), 0.021 / 0.023 (int_z300),
0.024 / 0.026 (int_z323), 0.037 / 0.033 (translate_unaligned, all three offsets), 0.029 / 0.029 (int_z60_unaligned); the
right-hand side b 0.014 - 0.563
(largest: iso2_gauss 0.530 / 0.563, identity 0.454 / 0.478, z_aniso 0.406 / 0.409); the objectives at most 0.022 of
their bound (dn_under64, central; 0.005 and below elsewhere); every dot inside the float64 summation's slack.  No
case failed: the table found no kernel bug.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (8, 4, 30)
SENT = -7.75e37  # sentinel of the pads around an unaligned output
NONFWD = ('backward', 'central')


def _c(kw, env=None, conc=1, expect=None, light=False, seed=11, unaligned=False, conv=None, tile=None, spacing=None,
       matvec=None):
    """``conv``: (kernels of conv.hip that must launch, those only A p alone launches, those that must not), by name
    with or without template arguments; ``tile``: where ``comb`` puts its deltas (default: the splat tile);
    ``spacing``: the y-space comb spacing where ``spacings`` is too narrow for the case's taps; ``matvec``: the
    one-kernel matvec form the case must run (``_mv``), checked by ``matvec_drift`` - a case that has one also runs
    the forward objectives."""
    return dict(kw=kw, env=env or {}, conc=conc, expect=expect, light=light, seed=seed, unaligned=unaligned,
                conv=conv, tile=tile, spacing=spacing, matvec=matvec)


def _mv(kernel, where=None, src='ata'):
    """A ``matvec`` entry.  ``kernel``: the instantiation's [matvec] name with '{}' where its DOT, OBJ arguments
    stand ('k_ata_shift_m<1,{},0>': NL = 1, not FAST), or None: no one-kernel form may launch; ``where``: a condition
    on the run-time facts of its line (a dict: grid, xr, lw, padl, padr, nf / padl, padr, nk, s); ``src``: the caller
    launch_lines reports ('ata': launch_ata_aligned, 'dtd': launch_dtd_lines; lines of shift.hip carry none)."""
    return dict(kernel=kernel, where=where, src=src)


_Z = dict(dim_y=(41, 38, 61), thick=6, thick_axes=[2], rot=0.1, trans=2.0, scl=0.1)
_DN = dict(dim_y=(41, 38, 61), regime='dn', rot=0.1, trans=2.0)
_MID = dict(dim_y=(97, 90, 121), thick=6, thick_axes=[2], rot=0.12, trans=2.0, scl=0.1)
_ISO = dict(dim_y=(42, 38, 61), thick=2, iso=(2, 2, 2), rot=0.1, trans=1.0, scl=0.1)
_oriented = lambda i: i['perm'] != (0, 1, 2) or any(i['flip'])

CASES = {
    'z_thick': _c(_MID, expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable']),
    'z_thick_conc3': _c(_MID, conc=3, expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable']),
    'x_thick': _c(dict(_Z, thick=4, thick_axes=[0]), expect=lambda i: i['pull2'] and i['splat2_axis'] == 0),
    'y_thick': _c(dict(_Z, thick=4, thick_axes=[1]), expect=lambda i: i['pull2'] and i['splat2_axis'] == 1),
    'iso2_rect': _c(_ISO, expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable']),
    'iso2_rect_z4': _c(dict(_ISO, dim_y=(42, 38, 64)),
                       expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable']),
    # (AXIS 3 carries the slice scaling along z only; with all ratios equal the thick axis is x: scl 0 here)
    'iso2_rect_nohyb': _c(dict(_ISO, scl=0.0), {'UNIRES_NO_HYBRID': '1'}, expect=lambda i: i['splat2_axis'] == 3),
    'iso2_gauss': _c(dict(dim_y=(34, 30, 36), thick=2, iso=(2, 2, 2), prof_ip=2, rot=0.1, trans=1.0),
                     expect=lambda i: i['separable']),
    'denoise': _c(_DN, expect=lambda i: i['fused']),
    'denoise_noata1': _c(_DN, {'UNIRES_NO_ATA1': '1'},
                         expect=lambda i: not i['fused'] and i['pull2'] and i['splat2_axis'] == -1),
    # (the shift kernel's domain: identity rotation, z profile only, dim_y.z a multiple of 4 in [8, 256])
    'translate': _c(dict(_Z, dim_y=(41, 38, 60), rot=0.0), expect=lambda i: i['shift']),
    'translate_noshift': _c(dict(_Z, dim_y=(41, 38, 60), rot=0.0), {'UNIRES_NO_SHIFT': '1'},
                            expect=lambda i: not i['shift']),
    'int_shift': _c(dict(_Z, shift=(2.0, -1.0, 3.0)), expect=lambda i: not i['shift'] and i['splat2_axis'] == 2),
    'int_shift_noalign': _c(dict(_Z, shift=(2.0, -1.0, 3.0)), {'UNIRES_NO_ALIGNED': '1'},
                            expect=lambda i: not i['shift']),
    # (z a multiple of 4: the shift kernel's tables are built for the integer shift too, and the 16-byte aligned forms
    # of the one-kernel matvecs are open to it)
    'int_shift_z60': _c(dict(_Z, dim_y=(41, 38, 60), shift=(2.0, -1.0, 3.0)), expect=lambda i: i['shift']),
    'identity': _c(dict(dim_y=(37, 41, 53), regime='id'), expect=lambda i: i['regime'] == 'identity'),
    'identity_noflat': _c(dict(dim_y=(37, 41, 53), regime='id'), {'UNIRES_NO_FLAT': '1'},
                          expect=lambda i: i['regime'] == 'identity'),
    'orient_9': _c(dict(_Z, thick=4, scl=0.0, orient=9),
                   expect=lambda i: _oriented(i) and i['pull2'] and i['splat2_axis'] is not None),
    'orient_22': _c(dict(_Z, thick=4, scl=0.0, orient=22),
                    expect=lambda i: _oriented(i) and i['pull2'] and i['splat2_axis'] is not None),
    'z_nosplat2': _c(_Z, {'UNIRES_NO_SPLAT2': '1'}, expect=lambda i: i['splat2_axis'] is None),
    'z_pushtile': _c(_Z, {'UNIRES_PUSH': 'tile'}, expect=lambda i: i['splat2_axis'] == 2),
    'z_nopull2': _c(_Z, {'UNIRES_NO_PULL2': '1'}, expect=lambda i: not i['pull2']),
    'dn_nopull2': _c(_DN, {'UNIRES_NO_PULL2': '1', 'UNIRES_NO_ATA1': '1'},
                     expect=lambda i: not i['pull2'] and not i['fused'] and i['splat2_axis'] == -1),
    'ctab_1266': _c(dict(dim_y=(24, 20, 1266), thick=6, thick_axes=[2], rot=0.02, trans=1.0),
                    expect=lambda i: i['splat2_axis'] == 2),
    'ctab_1272': _c(dict(dim_y=(24, 20, 1272), thick=6, thick_axes=[2], rot=0.02, trans=1.0),
                    expect=lambda i: i['splat2_axis'] is None),
    'rowcode_724': _c(dict(dim_y=(724, 724, 12), thick=6, thick_axes=[2], rot=0.02, trans=1.0), light=True,
                      expect=lambda i: i['splat2_axis'] == 2),
    'rowcode_725': _c(dict(dim_y=(725, 724, 12), thick=6, thick_axes=[2], rot=0.02, trans=1.0), light=True,
                      expect=lambda i: i['splat2_axis'] is None),
    'ax0_gdy511': _c(dict(dim_y=(24, 511, 20), thick=4, thick_axes=[0], rot=0.02, trans=1.0),
                     expect=lambda i: i['splat2_axis'] == 0),
    'ax0_gdy512': _c(dict(dim_y=(24, 512, 20), thick=4, thick_axes=[0], rot=0.02, trans=1.0),
                     expect=lambda i: i['splat2_axis'] is None),
    'ax1_gdy509': _c(dict(dim_y=(24, 508, 20), thick=4, thick_axes=[1], rot=0.02, trans=1.0),
                     expect=lambda i: i['splat2_axis'] == 1),
    'ax1_gdy513': _c(dict(dim_y=(24, 512, 20), thick=4, thick_axes=[1], rot=0.02, trans=1.0),
                     expect=lambda i: i['splat2_axis'] is None),
}

# The stride-2 conv passes across their block seams (the table in the module docstring).  Seeds are part of the case:
# with them the reference excludes no voxel as a FOV tie (tests/test_voxelwise_comparator.py holds them to that).
_S2 = dict(dim_y=(26, 70, 72), thick=2, iso=(2, 2, 2), rot=0.1, trans=1.0)
_S2G = dict(_S2, prof_ip=2, scl=0.05)
_S2R = dict(_S2, scl=0.1)
_S2Z = dict(dim_y=(24, 20, 256), thick=2, iso=(2, 2, 2), prof_ip=2, prof_tp=2, angles=(0, 0, 0.04), trans=1.0)
_sep = lambda i: i['separable']
_ONE_KERNEL = ['k_conv_ydown_xdownup2', 'k_conv1d_downup2_m', 'k_conv_up_yz2']
SEAM_CASES = {
    'sep2_gauss': _c(_S2G, seed=9, expect=_sep, tile=(12, 64, 64),
                     conv=(['k_conv_ydown_xdownup2<9,3,2,0>', 'k_conv_up_yz2<5>', 'k_conv1d_up2_m<2>'],
                           ['k_conv1d_down2_m<9>', 'k_conv1d_down2_m<3>'], ['k_conv1d_downup2_m'])),
    'sep2_gauss_noyx': _c(_S2G, {'UNIRES_CONV_YX': '0'}, seed=9, expect=_sep, tile=(16, 16, 64),
                          conv=(['k_conv1d_downup2_m<3,2>', 'k_conv1d_down2_m<9>', 'k_conv_up_yz2<5>'], [],
                                ['k_conv_ydown_xdownup2'])),
    'sep2_gauss_march': _c(_S2G, {'UNIRES_CONV_YX': '0', 'UNIRES_CONV_DOWNUP': '0', 'UNIRES_UPYZ_LDS': '0'}, seed=9,
                           expect=_sep, tile=(16, 16, 64),
                           conv=(['k_conv1d_down2_m<9>', 'k_conv1d_down2_m<3>', 'k_conv1d_up2_m<2>', 'k_conv1d_up2_m<5>',
                                  'k_conv1d_up_z2'], [], _ONE_KERNEL)),
    'sep2_gauss_tri': _c(dict(_S2, prof_ip=2, prof_tp=1), seed=9, expect=_sep, tile=(12, 64, 64),
                         conv=(['k_conv_ydown_xdownup2<9,5,3,0>', 'k_conv1d_up2_m<3>', 'k_conv_up_yz2<5>'],
                               ['k_conv1d_down2_m<5>', 'k_conv1d_down2_m<9>'], [])),
    'sep2_allgauss': _c(dict(_S2G, prof_tp=2), seed=9, expect=_sep, tile=(12, 64, 64),
                        conv=(['k_conv_ydown_xdownup2<9,9,5,0>', 'k_conv1d_up2_m<5>', 'k_conv_up_yz2<5>'],
                              ['k_conv1d_down2_m<9>'], [])),
    # (without a switch the z profile of such a plan rides in the window pull; k_conv1d_down_z runs where that declines)
    'sep2_allgauss_nopull2': _c(dict(_S2G, prof_tp=2), {'UNIRES_NO_PULL2': '1'}, seed=9, tile=(16, 16, 64),
                                expect=lambda i: i['separable'] and not i['pull2'],
                                conv=(['k_conv_up_yz2<5>', 'k_conv1d_up2_m<5>'], ['k_conv1d_down_z', 'k_conv1d_down2_m<9>'],
                                      ['k_conv_ydown_xdownup2', 'k_conv1d_downup2_m'])),
    'sep2_rect': _c(_S2R, seed=11, expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable'],
                    tile=(12, 62, 64),
                    conv=(['k_conv_ydown_xdownup2<3,3,2,2>', 'k_conv2d_up_xy_v4_t<2,2,4>'], ['k_conv2d_down_xy_v4'], [])),
    'sep2_rect_noxy': _c(_S2R, {'UNIRES_CONV_YX': '0', 'UNIRES_CONV_XY': '0'}, seed=11,
                         expect=lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable'], tile=(16, 16, 64),
                         conv=(['k_conv1d_down2_m<3>', 'k_conv1d_up2_m<2>'], [],
                               ['k_conv_ydown_xdownup2', 'k_conv2d_down_xy_v4', 'k_conv2d_up_xy_v4_t'])),
    'sep2_tri': _c(dict(_S2, prof_ip=1, prof_tp=1), seed=11, expect=_sep, tile=(12, 64, 64),
                   conv=(['k_conv_ydown_xdownup2<5,5,3,0>', 'k_conv2d_up_xy_v4_t<3,3,2>'], ['k_conv1d_down2_m<5>'], [])),
    'sep2_z256': _c(_S2Z, {'UNIRES_UPYZ_LDS': '0'}, seed=3, expect=_sep, tile=(8, 4, 244),
                    conv=(['k_conv1d_up_z2', 'k_conv1d_up2_m<5>'], [], ['k_conv_up_yz2'])),
    'sep2_z1024': _c(dict(_S2Z, dim_y=(24, 20, 1024)), seed=3, expect=_sep, tile=(8, 4, 244),
                     conv=(['k_conv_up_yz2<5>'], [], [])),
    'sep2_z1032': _c(dict(_S2Z, dim_y=(24, 20, 1032)), seed=3, expect=_sep, tile=(8, 4, 244),
                     conv=(['k_conv1d_up2_m<5>', 'k_conv1d_up_z2'], [], ['k_conv_up_yz2'])),
    'sep3_x150': _c(dict(dim_y=(150, 18, 24), thick=3, iso=(3, 3, 3), prof_ip=2, rot=0.05, trans=1.0), seed=1,
                    expect=_sep, tile=(144, 6, 12), spacing=(27, 33, 33),
                    conv=(['k_conv1d_up<float4>', 'k_conv1d_up_z'], ['k_conv1d_down<float4>'], [])),
    'sep3_x150_nopull2': _c(dict(dim_y=(150, 18, 24), thick=3, iso=(3, 3, 3), prof_ip=2, rot=0.05, trans=1.0),
                            {'UNIRES_NO_PULL2': '1'}, seed=1, expect=lambda i: i['separable'] and not i['pull2'],
                            tile=(144, 6, 12), spacing=(27, 33, 33),
                            conv=(['k_conv1d_up<float4>', 'k_conv1d_up_z'], ['k_conv1d_down_z', 'k_conv1d_down<float4>'],
                                  [])),
}
CASES.update(SEAM_CASES)

# Every one-kernel matvec form (shift.hip, aligned.hip) and the edges of their domains: the table in the module
# docstring.  Thick slices along z, no rotation, an exact translation (make_problem(shift=)), seed 11, scl 0.1.  The
# expected instantiation is read off launch_ata_shift / shift_nl / shift_xr / shift_fast / shift_build and launch_lines /
# launch_ata_aligned / launch_dtd_lines; the child's [matvec] lines (UNIRES_MATVEC_VERBOSE=1) must show it.
_FRAC, _INT = (0.3, -0.6, 0.4), (2.0, -1.0, 3.0)
_OKT = (4, 2, 64)  # the kernels' own seams: the x run (xr = 4 at these sizes), the pair of lines, the 4-voxel lane


def _ok(dim_y, thick, shift, matvec, expect=None, **kw):
    spacing = kw.pop('spacing', None)
    return _c(dict(dim_y=dim_y, thick=thick, thick_axes=[2], shift=shift, scl=0.1, **kw), expect=expect, tile=_OKT,
              spacing=spacing, matvec=matvec)


def _id(nz, matvec):
    return _c(dict(dim_y=(9, 8, nz), regime='id'), {'UNIRES_NO_FLAT': '1'}, expect=lambda i: i['regime'] == 'identity',
              tile=_OKT, matvec=matvec)


_shift, _noshift = (lambda i: i['shift']), (lambda i: not i['shift'])
_M2, _M1 = 'k_ata_shift_m<2,{},0>', 'k_ata_shift_m<1,{},0>'
ONE_KERNEL_CASES = {
    'tr_yodd': _ok((41, 37, 60), 6, _FRAC, _mv(_M1), _shift),
    'tr_yodd_z256': _ok((12, 9, 256), 6, (0.3, -0.6, 2.4), _mv('k_ata_shift_m<1,{},1>', lambda f: f['lw'] == 1), _shift),
    'int_yodd_z256': _ok((10, 11, 256), 6, _INT, _mv('k_ata_shift_m<1,{},1>', lambda f: f['lw'] == 1), _shift),
    'tr_thick2': _ok((20, 18, 40), 2, _FRAC, _mv(_M2, lambda f: f['nf'] == 4), _shift),
    # (a rect profile's taps are symmetric about their centre, so their count is odd: 3, 5, 5, 7 at ratio 2, 3, 4, 6 -
    # ratio 3 keeps five taps like ratio 4, nf = 6; no rect profile gives nf = 5.  nf = 6 and the triangle's 10 are the
    # counts that are no multiple of four)
    'tr_thick3': _ok((20, 18, 48), 3, _FRAC, _mv(_M2, lambda f: f['nf'] == 6), _shift),
    'tr_thick4': _ok((20, 18, 48), 4, _FRAC, _mv(_M2, lambda f: f['nf'] == 6), _shift),
    'tr_xdz128': _ok((12, 10, 256), 2, _FRAC, _mv(_M2, lambda f: f['lw'] == 0), _shift),
    'tr_zpos': _ok((20, 18, 60), 6, (0.3, -0.6, 9.6), _mv(_M2, lambda f: f['padr'] > 0), _shift),
    'tr_zneg': _ok((20, 18, 60), 6, (0.3, -0.6, -7.4), _mv(_M2, lambda f: f['padl'] >= 12), _shift),
    'tr_xyout': _ok((20, 18, 60), 6, (-3.3, 4.6, 0.4), _mv(_M2), _shift),
    'tr_z8': _ok((9, 6, 8), 2, _FRAC, _mv(_M2), _shift),
    'tr_x3': _ok((3, 4, 8), 2, _FRAC, _mv(_M2, lambda f: f['xr'] == 4), _shift),
    'tr_z260': _ok((9, 6, 260), 6, _FRAC, _mv(None), _noshift),
    'tr_x1028': _ok((1028, 6, 8), 2, _FRAC, _mv('k_ata_shift2<{}>', lambda f: f['xr'] == 0), _shift),
    'tr_x1028_yodd': _ok((1028, 5, 8), 2, _FRAC, _mv('k_ata_shift<{}>', lambda f: f['xr'] == 0), _shift),
    # (nine taps at stride 4: a fan-in of three x-space voxels - launch_ata_aligned declines (> 2), shift_build's
    # triples hold it; the default spacing (15, 15, 33) is wider than the nine taps' 2 (9 + 1) + 1 = 21, and is stated)
    'tr_tri4': _ok((20, 18, 48), 4, _FRAC, _mv(_M2, lambda f: f['nf'] == 10), _shift, prof_tp=1, spacing=(15, 15, 33)),
    'int_tri4': _ok((20, 18, 48), 4, _INT, _mv(_M2, lambda f: f['nf'] == 10), _shift, prof_tp=1, spacing=(15, 15, 33)),
    'int_yodd_z60': _ok((41, 37, 60), 6, _INT, _mv('k_ata_aligned4<1,{}>'), _shift),
    'int_z300': _ok((9, 8, 300), 6, _INT, _mv('k_ata_aligned4<2,{}>'), _noshift),
    'int_z203': _ok((9, 8, 203), 6, _INT, _mv('k_ata_aligned<4,{}>'), _noshift),
    'int_z323': _ok((9, 8, 323), 6, _INT, _mv('k_ata_aligned<6,{}>'), _noshift),
    'int_z451': _ok((9, 8, 451), 6, _INT, _mv('k_ata_aligned<8,{}>'), _noshift),
    'int_z512': _ok((9, 8, 512), 6, _INT, _mv('k_ata_aligned4<2,{}>'), _noshift),
    'int_z516': _ok((9, 8, 516), 6, _INT, _mv(None), _noshift),
    'int_zneg': _ok((20, 18, 61), 6, (2.0, -1.0, -5.0), _mv('k_ata_aligned<2,{}>', lambda f: f['padl'] > 1), _noshift),
    'int_zpos': _ok((20, 18, 61), 6, (2.0, -1.0, 9.0), _mv('k_ata_aligned<2,{}>', lambda f: f['padr'] > 1), _noshift),
    'id_z203': _id(203, _mv('k_ata_aligned<4,{}>', src='dtd')),
    'id_z323': _id(323, _mv('k_ata_aligned<6,{}>', src='dtd')),
    'id_z451': _id(451, _mv('k_ata_aligned<8,{}>', src='dtd')),
    'id_z516': _id(516, _mv(None)),
}
CASES.update(ONE_KERNEL_CASES)

# The rotation sweep: the form each geometry runs at each angle, as observed on an MI355X: (pull2, splat2 axis,
# k_ata1, schedule build).  Without any env switch: from 0.3 rad on, a tile overflows its 128-entry staging slot
# and the schedule takes the two-pass build (up to 48 instructions per tile); at 0.7 rad a tile needs more than
# 64 instructions and splat2 (and k_ata1) leave their domain; at 0.78 rad about x the pull window leaves pull2's.
SWEEP_ANGLES = (0.3, 0.5, 0.7, 0.78)
_T, _F = True, False
SWEEP_FORMS = {
    'sweep_z_x0.30': (_T, 2, _F, 'two-pass'), 'sweep_z_x0.50': (_T, 2, _F, 'two-pass'),
    'sweep_z_x0.70': (_T, None, _F, None), 'sweep_z_x0.78': (_F, None, _F, None),
    'sweep_z_y0.30': (_T, 2, _F, 'two-pass'), 'sweep_z_y0.50': (_T, 2, _F, 'two-pass'),
    'sweep_z_y0.70': (_T, None, _F, None), 'sweep_z_y0.78': (_T, None, _F, None),
    'sweep_dn_x0.30': (_T, -1, _T, 'two-pass'), 'sweep_dn_x0.50': (_T, -1, _T, 'two-pass'),
    'sweep_dn_x0.70': (_T, None, _F, None), 'sweep_dn_x0.78': (_F, None, _F, None),
    'sweep_dn_y0.30': (_T, -1, _T, 'two-pass'), 'sweep_dn_y0.50': (_T, -1, _T, 'two-pass'),
    'sweep_dn_y0.70': (_T, None, _F, None), 'sweep_dn_y0.78': (_T, None, _F, None),
}
for _g, _kw in (('z', dict(_Z, scl=0.0)), ('dn', _DN)):
    for _ax in ('x', 'y'):
        for _a in SWEEP_ANGLES:
            _ang = (_a, 0.0, 0.0) if _ax == 'x' else (0.0, _a, 0.0)
            CASES['sweep_%s_%s%.2f' % (_g, _ax, _a)] = _c(dict(_kw, angles=_ang))
# every case below 0.3 rad builds its schedule in one pass: the staging slot holds its tiles
for _n in CASES:
    if not _n.startswith('sweep_'):
        CASES[_n]['one_pass'] = True

# The table with a non-forward D (sett.diff = 'backward' / 'central'): the smallest shapes that still select each form
# the matvec of such a plan chooses between (api_operator.hip, matvec), by name from the table above where
# it has them, and the shapes where the closing stencil pass turns: anisotropic voxels (cx != cy != cz), two repeats
# (the accumulating stores), the k_dtd fallback of the flat kernel (fewer than 64 voxels; nz < 4) and an output 4, 8
# and 12 bytes off a 16-byte boundary.  No conv-table / row-code / grid limits and no sweep: those exercise the
# schedule, not the epilogue.
_ANISO = (0.8, 1.25, 2.0)
_z_form = lambda i: i['pull2'] and i['splat2_axis'] == 2 and not i['separable']
DIFF_CASES = {
    'z_thick': _c(_Z, expect=_z_form),
    'z_thick_conc3': _c(_Z, conc=3, expect=_z_form),
}
for _n in ('x_thick', 'y_thick', 'iso2_rect', 'iso2_rect_nohyb', 'iso2_gauss', 'denoise', 'denoise_noata1',
           'translate', 'translate_noshift', 'int_shift', 'int_shift_noalign', 'int_shift_z60', 'identity', 'orient_9',
           'z_nosplat2', 'z_pushtile', 'z_nopull2', 'dn_nopull2', 'sep2_gauss', 'sep2_rect'):
    DIFF_CASES[_n] = CASES[_n]
DIFF_CASES.update({
    'z_aniso': _c(dict(_Z, aniso=_ANISO), expect=_z_form),
    'dn_aniso': _c(dict(_DN, aniso=_ANISO), expect=lambda i: i['fused']),
    'sr_2rep': _c(dict(dim_y=(41, 38, 61), thick=4, n_repeats=2, rot=0.1, trans=2.0, scl=0.1),
                  expect=lambda i: i['pull2'] and i['splat2_axis'] is not None),
    'dn_2rep': _c(dict(dim_y=(21, 19, 33), regime='dn', n_repeats=2, rot=0.1, trans=2.0)),
    # (tests/test_gpu_ata1.py's dn_thin: 30 voxels, below the flat kernel's 64: k_dtd<ACC> closes the matvec)
    'dn_under64': _c(dict(dim_y=(3, 2, 5), regime='dn', rot=0.05, trans=0.3), seed=5),
    'dn_nz3': _c(dict(dim_y=(12, 10, 3), regime='dn', rot=0.1, trans=1.0)),  # (nz < 4: the same fallback)
    # 256-voxel lines: the x-marching shift kernel's fast form (shift.hip shift_fast: only there), which a one-repeat
    # plan tries first - a fractional and an integer shift (tests/test_gpu_path.py's sr_shift_z256 / sr_aligned_z256
    # geometries).  repeat_info shows that the shift tables exist, not which form of the kernel runs.
    'translate_z256': _c(dict(dim_y=(12, 10, 256), thick=6, thick_axes=[2], rot=0.0, trans=2.3, scl=0.1),
                         expect=lambda i: i['shift']),
    'int_shift_z256': _c(dict(dim_y=(10, 12, 256), thick=6, thick_axes=[2], shift=(2.0, -1.0, 3.0), scl=0.05),
                         expect=lambda i: i['shift']),
    'z_unaligned': _c(_Z, expect=_z_form, unaligned=True),
    'dn_unaligned': _c(_DN, expect=lambda i: i['fused'], unaligned=True),
})
# the one-kernel forms under a non-forward D: zero stencil weights, no partials (the <0,0> instantiations),
# stencil_close behind them - the marching kernel with one line per wave, the two fallbacks of x > 1024, the triple
# form of the z operator, a right apron, and three instantiations of aligned.hip
for _n in ('tr_yodd', 'tr_x1028', 'tr_x1028_yodd', 'tr_xdz128', 'tr_zpos', 'int_yodd_z60', 'int_z300', 'int_z323'):
    DIFF_CASES[_n] = ONE_KERNEL_CASES[_n]
# q 4, 8 and 12 bytes off a 16-byte boundary: launch_ata_shift declines (the fractional shift then takes the general
# pair: no one-kernel line) and launch_lines leaves its 16-byte forms for the dword one
DIFF_CASES['translate_unaligned'] = dict(CASES['translate'], unaligned=True, matvec=_mv(None))
DIFF_CASES['int_z60_unaligned'] = dict(CASES['int_shift_z60'], unaligned=True, matvec=_mv('k_ata_aligned<2,{}>'))

_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_voxelwise import comb, inputs, spacings
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan
kw, conc, light, out = %(kw)r, %(conc)r, %(light)r, sys.argv[1]
seed, diffs, unaligned, tile, spacing = %(seed)r, %(diffs)r, %(unaligned)r, %(tile)r, %(spacing)r
fwd_obj = %(fwd_obj)r
if 'orient' in kw:
    kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
prob = make_problem(seed=seed, **kw)
xg, yg, sett = gpu_structs(prob, 'cuda:0')
vx = N.voxel_size(prob['mat_y']).float()
plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
plan.set_concurrency(conc)
info = plan.repeat_info(0)
info['regime'] = 'identity' if not prob['do_proj'] else prob['method']
p, v = inputs(prob['dim_y'], plan.dims_x[0])
res = dict(info=json.dumps(info))
d = lambda t: t.to('cuda:0')
if prob['do_proj'] and 'forward' in diffs:
    sy, sx = spacings(kw, spacing)
    res['Ap'] = plan.proj_apply(0, 'A', d(p)).cpu().numpy()
    res['AtAp'] = plan.proj_apply(0, 'AtA', d(p)).cpu().numpy()
    if not light:
        res['Atv'] = plan.proj_apply(0, 'At', d(v)).cpu().numpy()
    for ph in (0, 1):
        pc = comb(prob['dim_y'], tile, sy, ph)
        res['AtA_comb%%d' %% ph] = plan.proj_apply(0, 'AtA', d(pc)).cpu().numpy()
        if not light:
            res['A_comb%%d' %% ph] = plan.proj_apply(0, 'A', d(pc)).cpu().numpy()
            vc = comb(plan.dims_x[0], None, sx, ph)
            res['At_comb%%d' %% ph] = plan.proj_apply(0, 'At', d(vc)).cpu().numpy()
rho, lam, n = prob['rho'], yg[0].lam, p.numel()
if 'forward' in diffs:
    dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
    res['q'] = plan.matvec(d(p), rho, lam, dot=dot).cpu().numpy()
    torch.cuda.synchronize()
    res['dot'] = np.array(dot.item())
for which in diffs:
    if which == 'forward' and not (fwd_obj and prob['do_proj']):
        continue
    if which != 'forward':
        plan.set_diff(which)
    # out=: a view 1, 2, 3 floats into a sentinel-padded buffer (q 4, 8, 12 bytes off a 16-byte boundary), else None
    for off in (() if which == 'forward' else (1, 2, 3) if unaligned else (0,)):
        tag = '%%s_off%%d' %% (which, off) if unaligned else which
        dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
        buf = torch.full((n + 8,), SENT, dtype=torch.float32, device='cuda:0')
        view = buf[off:off + n].view(prob['dim_y'])
        q = plan.matvec(d(p), rho, lam, out=view if unaligned else None, dot=dot)
        torch.cuda.synchronize()
        res['q_' + tag] = q.cpu().numpy()
        res['dot_' + tag] = np.array(dot.item())
        if unaligned:
            res['pads_' + tag] = np.array(bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all()))
    print('[phase] solve', file=sys.stderr, flush=True)  # (what follows runs on 16-byte aligned vectors of its own)
    b = plan.rhs([xn.dat for xn in xg[0]], d(prob['w'][0]), d(prob['z'][0]), rho, lam)
    res['b_' + which] = b.cpu().numpy()
    if prob['do_proj']:
        # a 'max_gain' solve of one iteration from x0 = p: trace[0] is the objective at p.  'max_gain' takes iteration
        # 1's objective from the recurred residual (unires_amd/_lib.py STOP); 'max_gain_fresh' evaluates it by the
        # matvec's objective epilogue, on the iterate the solve leaves in x: trace[1] of a second such solve
        x = d(p).clone()
        it, trace = plan.cg(b, x, rho, lam, max_iter=1, tolerance=1e-3, stop='max_gain')
        torch.cuda.synchronize()
        res['obj0_' + which] = np.array(trace[0])
        x = d(p).clone()
        it, trace = plan.cg(b, x, rho, lam, max_iter=1, tolerance=1e-3, stop='max_gain_fresh')
        torch.cuda.synchronize()
        if it >= 1:
            res['obj1_' + which] = np.array(trace[1])
            res['x1_' + which] = x.cpu().numpy()
            res['q1_' + which] = plan.matvec(x, rho, lam).cpu().numpy()  # (stored: for the error in tied voxels)
np.savez(out, **res)
'''.replace('SENT', repr(SENT))


def inputs(dim_y, dim_x):
    gen = torch.Generator().manual_seed(7)
    p = (torch.rand(tuple(dim_y), generator=gen) * 10 - 2).float()
    v = (torch.rand(tuple(dim_x), generator=gen) * 10 - 2).float()
    return p, v


def spacings(kw, spacing=None):
    """Comb spacing per axis, wider than the operator's footprint: y space 2 (3 r + 4) + 1 (A^T A reaches the
    conv taps (r + 3 at most for the rect profile, r + 3 + r for the Gaussian at ratio 2) plus a corner either
    side, twice), x space 8 (rows of A whose y footprints overlap).  ``spacing``: the case's own y-space spacing, for
    profiles with more taps (2 (taps + 1) + 1 of the taps the plan keeps: the Gaussian at ratio 3 has 15)."""
    r = [1, 1, 1]
    if kw.get('regime', 'sr') == 'sr':
        if kw.get('iso'):
            r = list(kw['iso'])
        else:
            r[kw['thick_axes'][0]] = kw['thick']
    return tuple(spacing) if spacing else tuple(2 * (3 * ri + 4) + 1 for ri in r), (8, 8, 8)


def comb(dim, tile, spacing, phase):
    """Deltas (random values) on the product of per-axis positions: the ends, the first / last voxel of the first
    and last (partial) tile and the middle, kept greedily in a phase-dependent order where at least ``spacing``
    from those already kept (phase 0 and 1 together cover both voxels of each adjacent pair)."""
    gen = torch.Generator().manual_seed(13 + phase)
    pos = []
    for a, n in enumerate(dim):
        t = tile[a] if tile is not None else max(1, n // 3)
        last = (n - 1) // t * t
        pri = ([0, last, t, n // 2, n - 1, last - 1, t - 1, 1] if phase == 0 else
               [n - 1, last - 1, t - 1, 1, n // 2, 0, last, t])
        keep = []
        for i in pri:
            if 0 <= i < n and all(abs(i - k) >= spacing[a] for k in keep):
                keep.append(i)
        pos.append(sorted(keep))
    out = torch.zeros(tuple(dim))
    for i in pos[0]:
        for j in pos[1]:
            for k in pos[2]:
                out[i, j, k] = float(torch.rand((), generator=gen)) * 4 + 1
    return out


def _run_child(tmp_path, name, case, diffs=('forward',), timeout=300):
    """One child process for the case; ``diffs``: the differences whose matvec it runs (non-forward ones also the
    right-hand side and a one-iteration solve)."""
    path = str(tmp_path / ('%s.npz' % name))
    env = dict(os.environ)
    env.update(case['env'])
    env['UNIRES_SPLAT2_VERBOSE'] = '1'
    env['UNIRES_CONV_VERBOSE'] = '1'
    env['UNIRES_MATVEC_VERBOSE'] = '1'
    r = subprocess.run([sys.executable, '-c', _CHILD % dict(root=ROOT, kw=case['kw'], conc=case['conc'],
                                                            light=case['light'], seed=case['seed'],
                                                            diffs=tuple(diffs), unaligned=case['unaligned'],
                                                            tile=case['tile'] or TILE, spacing=case['spacing'],
                                                            fwd_obj=case['matvec'] is not None), path],
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
    res = dict(np.load(path))
    builds = re.findall(r'\[splat2\].*build (\S+), max instructions per tile (\d+)', r.stderr)
    convs = set(re.findall(r'^\[conv\] (\S+)', r.stderr, re.M))
    return res, (builds[-1] if builds else None), convs, matvec_lines(r.stderr)


def matvec_lines(stderr):
    """The [matvec] lines of a child (UNIRES_MATVEC_VERBOSE=1), in order: (name, facts) with the name as printed
    ('k_ata_shift_m<1,1,0,1>') and the facts a dict of the integers beside it, 'src' the caller launch_lines names,
    'solve' whether the child had reached its first right-hand side and solve (a line is printed once, where its
    instantiation first launches: the matvecs into an unaligned ``out`` of the first difference come before)."""
    out, solve = [], False
    for kind, line in re.findall(r'^\[(matvec|phase)\] (.*)$', stderr, re.M):
        if kind == 'phase':
            solve = True
            continue
        tok = line.split()
        facts, i = {'src': None, 'solve': solve}, 1
        while i < len(tok):
            if tok[i] in ('ata', 'dtd'):
                facts['src'], i = tok[i], i + 1
            else:
                facts[tok[i]], i = int(tok[i + 1]), i + 2
        out.append((tok[0], facts))
    return out


def matvec_drift(case, lines, forward=True, proj=True):
    """The case's ``matvec`` expectation against the [matvec] lines of its child: a list of misses.  With forward
    differences the named form must have run with the dot (DOT, OBJ = 1, 0) and, where the child solves (A != I), as
    the fresh objective (1, 1); with a non-forward D every one-kernel launch must be the plain form (0, 0: zero
    stencil weights, no partials - stencil_close finishes the matvec), the named one among them.  Every launch of
    the named form must meet ``where`` and come from ``src``; no other one-kernel form may launch.  An ``unaligned``
    case states the form of its matvecs into the unaligned ``out``: the expectation holds for the lines from before
    the first solve, and the solves (on aligned vectors, so on the aligned forms) must still be plain."""
    mv = case['matvec']
    if mv is None:
        return []
    if case['unaligned']:
        late = [('run in a solve', n) for n, f in lines if f['solve'] and not re.search(r'<(\d,)?0,0(,\d)?>$', n)]
        return late + matvec_drift(dict(case, unaligned=False), [l for l in lines if not l[1]['solve']], forward, proj)
    if mv['kernel'] is None:
        return [('run', n) for n, _ in lines]
    want = (['1,0', '1,1'] if proj else ['1,0']) if forward else ['0,0']
    allowed = ['1,0', '1,1', '0,0'] if forward else ['0,0']
    names = [n for n, _ in lines]
    miss = [('not run', mv['kernel'].format(a)) for a in want if mv['kernel'].format(a) not in names]
    for n, facts in lines:
        if n not in [mv['kernel'].format(a) for a in allowed]:
            miss.append(('run', n))
        elif mv['where'] is not None and not mv['where'](facts):
            miss.append(('facts', n, facts))
        elif n.startswith('k_ata_aligned') and facts['src'] != mv['src']:
            miss.append(('caller', n, facts['src']))
    return miss


def obj_check(name, key, got, x, b64, q_ref, q_tol, q_err_ties):
    """An objective 0.5 sum_v obj_term(q_v, b_v, x_v) against float64 (``_check_diff`` derives the bound): asserts, and
    returns err / tol."""
    from tests import ref64
    x64 = x.double().abs()
    want = 0.5 * float(((q_ref - 2 * b64) * x.double()).sum())
    tol = 0.5 * float((x64 * (q_tol + 3 * ref64.U * (q_ref.abs() + 2 * b64.abs()))).sum()) + 0.5 * q_err_ties
    assert abs(got - want) <= tol, (name, key, got, want, tol)
    return abs(got - want) / tol


def conv_drift(case, convs, forward=True):
    """The case's ``conv`` expectation against the [conv] names of its child: a list of (what, name) misses.  A name
    without template arguments stands for every instantiation.  ``forward``: the child ran A p on its own."""
    if case['conv'] is None:
        return []
    run, fwd, no = case['conv']
    hit = lambda name: any(c == name or c.startswith(name + '<') for c in convs)
    return ([('not run', n) for n in run + (fwd if forward else []) if not hit(n)] +
            [('run', n) for n in no if hit(n)])


def _check(name, case, res):
    from oracle import nitorch_restated as N
    from oracle import unires_restated as O
    from tests import ref64
    from tests.helpers import SIGNED_PERMS, make_problem, oracle_structs
    kw = case['kw']
    if 'orient' in kw:
        kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
    prob = make_problem(seed=case['seed'], **kw)
    xs, ys = oracle_structs(prob)
    xc, yc = xs[0], ys[0]
    info = json.loads(str(res['info']))
    vx = N.voxel_size(prob['mat_y']).float()
    rho = torch.tensor(prob['rho'], dtype=torch.float32)
    p, v = inputs(prob['dim_y'], xc[0].po.dim_x if prob['do_proj'] else prob['dim_y'])
    p64 = p.double()
    q = torch.from_numpy(res['q'])
    rep = {}

    def dot_ok(refq, tolq, ex):
        err_q = (q.double() - refq).abs()
        slack = float((p64.abs() * err_q)[ex].sum()) if ex is not None else 0.0
        return abs(float(res['dot']) - float((p64 * refq).sum())) <= float((p64.abs() * tolq).sum()) + slack

    if not prob['do_proj']:  # A = I: q = tau p + rho lam^2 DtD p
        tau = float(torch.tensor(float(xc[0].tau), dtype=torch.float32))
        lam = float(torch.tensor(float(yc.lam), dtype=torch.float32))
        c = float(rho) * lam * lam
        refq = tau * p64 + c * O.DtD(p64, vx)
        tolq = (ref64.U + ref64.U64) * (ref64.C_DTD + 2) * (tau * p64.abs() + c * ref64.dtd_abs(p64.abs(), vx))
        r = ref64.compare(q, refq, tolq)
        assert r['ok'], (name, 'matvec', r)
        assert dot_ok(refq, tolq, None), (name, 'dot')
        rep['matvec'] = r['max_ratio']
        return rep, 0, 0.0
    # the bound's orientation (it widens the coordinate error) is restated, and must be the plan's
    mat, _ = O.proj_matrix(xc[0].po, prob['method'])
    perm, flip, oriented = ref64.orientation_of(mat.float().double())
    assert (tuple(info['perm']), tuple(info['flip'])) == (perm, flip), (name, info, perm, flip)
    op = ref64.Operator64(xc[0].po, prob['method'], oriented=oriented)
    mx, my, myy, n_near = op.tie_masks(xc[0].po)
    assert int(myy.sum()) < 0.01 * p.numel(), (name, int(myy.sum()))
    refA, tolA = op.bound_A(p)
    r = ref64.compare(torch.from_numpy(res['Ap']), refA, tolA, mx)
    assert r['ok'], (name, 'A', r)
    rep['A'] = r['max_ratio']
    ref, tol = op.bound_AtA(p)
    r = ref64.compare(torch.from_numpy(res['AtAp']), ref, tol, myy)
    assert r['ok'], (name, 'AtA', r)
    rep['AtA'] = r['max_ratio']
    del ref, tol
    refq, tolq = op.bound_matvec(p, xc[0].tau, rho, yc.lam, vx)
    r = ref64.compare(q, refq, tolq, myy)
    assert r['ok'], (name, 'matvec', r)
    rep['matvec'] = r['max_ratio']
    # the float64 dot epilogue: <p, q> within sum |p| tol_q (+ the actual error in tied voxels)
    assert dot_ok(refq, tolq, myy), (name, 'dot')
    if case['matvec'] is not None:
        # the forward objectives of the one-kernel forms (``_check_diff``'s entries 0 and 1, with forward differences:
        # entry 1 of the 'max_gain_fresh' solve is the kernel's own OBJ instantiation, the data term from registers)
        b64 = torch.from_numpy(res['b_forward']).double()
        ties = float((p64.abs() * (q.double() - refq).abs())[myy].sum())
        rep['obj0'] = obj_check(name, 'obj0_forward', float(res['obj0_forward']), p, b64, refq, tolq, ties)
        assert 'obj1_forward' in res, (name, 'the solve ran no iteration')
        x1 = torch.from_numpy(res['x1_forward'])
        ref1, tol1 = op.bound_matvec(x1, xc[0].tau, rho, yc.lam, vx)
        tie1 = float((x1.double().abs() * (torch.from_numpy(res['q1_forward']).double() - ref1).abs())[myy].sum())
        rep['obj1'] = obj_check(name, 'obj1_forward', float(res['obj1_forward']), x1, b64, ref1, tol1, tie1)
        del ref1, tol1
    del refq, tolq
    if not case['light']:
        refAt, tolAt = op.bound_At(v)
        r = ref64.compare(torch.from_numpy(res['Atv']), refAt, tolAt, my)
        assert r['ok'], (name, 'At', r)
        rep['At'] = r['max_ratio']
        # the float64 adjoint identity on the kernels' A and At
        Ap, Atv, v64 = torch.from_numpy(res['Ap']).double(), torch.from_numpy(res['Atv']).double(), v.double()
        lhs = abs(float((Ap * v64).sum()) - float((p64 * Atv).sum()))
        slack = float(((Ap - refA).abs() * v64.abs())[mx].sum() + ((Atv - refAt).abs() * p64.abs())[my].sum())
        assert lhs <= float((tolA * v64.abs()).sum() + (tolAt * p64.abs()).sum()) + slack, (name, 'adjoint')
    # impulse combs against the plan's own taps (D = 0): columns of A and AtA, rows of A via At
    opt = ref64.Operator64(xc[0].po, prob['method'], trimmed=True, oriented=oriented)
    sy, sx = spacings(case['kw'], case['spacing'])
    for ph in (0, 1):
        pc = comb(prob['dim_y'], case['tile'] or TILE, sy, ph)
        checks = [('AtA_comb%d' % ph, lambda: opt.bound_AtA(pc), myy)]
        if not case['light']:
            vc = comb(tuple(xc[0].po.dim_x), None, sx, ph)
            checks += [('A_comb%d' % ph, lambda: opt.bound_A(pc), mx), ('At_comb%d' % ph, lambda: opt.bound_At(vc), my)]
        for key, bound, ex in checks:
            refc, tolc = bound()
            r = ref64.compare(torch.from_numpy(res[key]), refc, tolc, ex)
            assert r['ok'], (name, key, r)
            rep[key] = r['max_ratio']
    return rep, int(myy.sum()), op.R


def test_every_form_per_voxel_against_float64(tmp_path):
    drift = []
    for name, case in CASES.items():
        res, build, convs, mvs = _run_child(tmp_path, name, case)
        info = json.loads(str(res['info']))
        info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
        form = (info['pull2'], info['splat2_axis'], info['fused'], build[0] if build else None)
        if case['expect'] is not None and not case['expect'](info):
            drift.append((name, info))  # (checked after the table: every case's form is reported)
        if case.get('one_pass') and build is not None and build[0] != 'one-pass':
            drift.append((name, build))
        if name in SWEEP_FORMS and SWEEP_FORMS[name] != form:
            drift.append((name, form, SWEEP_FORMS[name]))
        if conv_drift(case, convs):
            drift.append((name, conv_drift(case, convs), sorted(convs)))
        mdrift = matvec_drift(case, mvs, proj=info['regime'] != 'identity')
        if mdrift:
            drift.append((name, mdrift, mvs))
        rep, excluded, R = _check(name, case, res)
        print('%-20s %s build %s conv %s max err/tol %.3f excluded %d R %.0f'
              % (name, info, build, ' '.join(sorted(convs)) or '-', max(rep.values()), excluded, R), flush=True)
        for n, facts in mvs:
            print('%-20s [matvec] %s %s' % (name, n, ' '.join('%s %s' % kv for kv in facts.items() if kv[1] not in (None, True, False))),
                  flush=True)
        if case['matvec'] is not None and 'obj0' in rep:
            print('%-20s obj0 %.4f obj1 %.4f of their bound' % (name, rep['obj0'], rep['obj1']), flush=True)
    assert not drift, drift


def diff_reference(case):
    """The float64 side of a case of DIFF_CASES, everything that does not depend on the difference: the problem, one
    Operator64 per repeat (None with A = I), the unions of the repeats' tie masks (``my`` for the right-hand side,
    ``myy`` for the matvec), the inputs, and the repeats' A^T A parts of p and A^T bounds of their observations."""
    from oracle import nitorch_restated as N
    from oracle import unires_restated as O
    from tests import ref64
    from tests.helpers import SIGNED_PERMS, make_problem, oracle_structs
    kw = case['kw']
    if 'orient' in kw:
        kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
    prob = make_problem(seed=case['seed'], **kw)
    xs, ys = oracle_structs(prob)
    xc, yc = xs[0], ys[0]
    R = dict(prob=prob, xc=xc, yc=yc, vx=N.voxel_size(prob['mat_y']).float(), taus=[xn.tau for xn in xc],
             rho=torch.tensor(prob['rho'], dtype=torch.float32))
    R['p'] = inputs(prob['dim_y'], prob['dim_y'])[0]
    n = R['p'].numel()
    R['my'] = torch.zeros(prob['dim_y'], dtype=torch.bool)
    R['myy'] = R['my'].clone()
    if not prob['do_proj']:
        R['ops'] = [None] * len(xc)
        return R
    R['ops'], R['orient'] = [], []
    for xn in xc:
        mat, _ = O.proj_matrix(xn.po, prob['method'])
        perm, flip, oriented = ref64.orientation_of(mat.float().double())
        op = ref64.Operator64(xn.po, prob['method'], oriented=oriented)
        _, my, myy, _ = op.tie_masks(xn.po)
        R['ops'].append(op)
        R['orient'].append((perm, flip))
        R['my'] |= my
        R['myy'] |= myy
    return R


def tie_cap_ok(R):
    """The cap on excluded voxels: fewer than 1 % of the volume (none in a volume below 100 voxels)."""
    n = R['p'].numel()
    return int(R['myy'].sum()) < 0.01 * n and int(R['my'].sum()) < 0.01 * n


def _check_diff(name, case, res, R):
    """Matvec, dot, right-hand side and the objectives of one-iteration solves, for both non-forward differences of
    one case.

    The objective (cg.hip): entry k of the trace is 0.5 sum_v obj_term(q_v, b_v, x_v) over the iterate x of iteration
    k, q = A(x) the plan's matvec of it, with obj_term = fl(fl(q - fl(2 b)) x): three float32 operations, of which the
    doubling is exact; each of the other two is off by at most u times its result, at most u (|q| + 2 |b|) |x|; the
    bound below counts all three.  Entry 0 (obj0, of a 'max_gain' solve) is formed by k_residual_init from the q the
    start's matvec stored (the closing pass in its ACC form without an epilogue).  Entry 1 of a 'max_gain' solve is
    taken from the recurred residual, not from a matvec; obj1 is entry 1 of a 'max_gain_fresh' solve, formed by the
    objective epilogue of the closing pass (ACC and OBJ: the data term read from q, nothing stored), on the iterate
    x1 that solve leaves in x.  So for x = p
    (entry 0) and x = x1 (entry 1), with (refq, tolq) the float64 matvec of the stored x and b the stored
    right-hand side:

        |obj - 0.5 sum (refq - 2 b) x| <= 0.5 sum |x| (tolq + 3 u (|refq| + 2 |b|)) + 0.5 sum_ties |x| |q - refq|

    where the last term is the actual error of the kernel's q in tied voxels (entry 1: of the q a stored matvec of x1
    returns - the same kernels on the same coordinates, so the same FOV decisions)."""
    from tests import diff64, ref64
    prob, ops, taus, rho, lam, vx = R['prob'], R['ops'], R['taus'], R['rho'], R['yc'].lam, R['vx']
    p, my, myy = R['p'], R['my'], R['myy']
    p64 = p.double()
    proj = prob['do_proj']
    assert tie_cap_ok(R), (name, int(myy.sum()), int(my.sum()))
    if proj and 'parts' not in R:
        R['parts'] = [op.parts_AtA(p) for op in ops]
        R['at'] = [op.bound_At(xn.dat) for op, xn in zip(ops, R['xc'])]
    offs = (1, 2, 3) if case['unaligned'] else (0,)
    rep, qs = {}, {}
    for which in NONFWD:
        if proj:
            refq, tolq = ref64.bound_matvec_reps(ops, taus, p, rho, lam, vx, which, parts=R['parts'])
        else:  # A = I: q = (sum tau) p + rho lam^2 DtD p, tests/diff64.py's bound for it
            a0 = np.float32(0.0)
            for t in taus:
                a0 = a0 + np.float32(float(t))
            c = np.float32(float(rho)) * (np.float32(float(lam)) * np.float32(float(lam)))
            refq, tolq = (torch.from_numpy(a) for a in diff64.a_plus_c_dtd(p.numpy(), vx.tolist(), which, a0, c))
        for off in offs:
            tag = '%s_off%d' % (which, off) if case['unaligned'] else which
            q = torch.from_numpy(res['q_' + tag])
            r = ref64.compare(q, refq, tolq, myy)
            assert r['ok'], (name, 'matvec', tag, r)  # (a voxel left at the sentinel is off by 7.75e37)
            assert torch.isfinite(q).all() and float(q.abs().max()) < 1e30, (name, 'unwritten voxel', tag)
            rep['q ' + tag] = r['max_ratio']
            if case['unaligned']:
                assert bool(res['pads_' + tag]), (name, 'pads', tag)
            # the dot's terms are exact products of the stored float32 values: the float64 dot of p and q as stored,
            # within the float64 summation's own slack
            want = float((p64 * q.double()).sum())
            slack = (p.numel() + 32) * 2.0 ** -53 * float((p64 * q.double()).abs().sum())
            assert abs(float(res['dot_' + tag]) - want) <= slack, (name, 'dot', tag, float(res['dot_' + tag]), want)
        qs[which] = q
        b = torch.from_numpy(res['b_' + which])
        refb, tolb = ref64.bound_rhs(ops, taus, [xn.dat for xn in R['xc']], prob['w'][0], prob['z'][0], rho, lam, vx,
                                     which, at=R.get('at'))
        r = ref64.compare(b, refb, tolb, my)
        assert r['ok'], (name, 'rhs', which, r)
        rep['b ' + which] = r['max_ratio']
        if not proj:
            continue
        b64 = b.double()
        ties = float((p64.abs() * (q.double() - refq).abs())[myy].sum())
        rep['obj0 ' + which] = obj_check(name, 'obj0_' + which, float(res['obj0_' + which]), p, b64, refq, tolq, ties)
        assert 'obj1_' + which in res, (name, 'the solve ran no iteration', which)
        x1 = torch.from_numpy(res['x1_' + which])
        ref1, tol1 = ref64.bound_matvec_reps(ops, taus, x1, rho, lam, vx, which)
        tie1 = float((x1.double().abs() * (torch.from_numpy(res['q1_' + which]).double() - ref1).abs())[myy].sum())
        rep['obj1 ' + which] = obj_check(name, 'obj1_' + which, float(res['obj1_' + which]), x1, b64, ref1, tol1, tie1)
    assert not torch.equal(qs['backward'], qs['central']), name
    return rep, int(myy.sum()), int(my.sum())


_DIFF_DEAD = []  # set by the first child that exits non-zero or times out: nothing more runs on the GPU after it


@pytest.mark.parametrize('name', list(DIFF_CASES))
def test_every_form_per_voxel_with_backward_and_central_differences(tmp_path, name):
    """Every form of DIFF_CASES with sett.diff = 'backward' and 'central': the matvec q per voxel against
    ref64.bound_matvec_reps, its dot, the right-hand side b per voxel against ref64.bound_rhs, and the first two
    objectives of a 'max_gain' solve (``_check_diff``).  One child per case, both differences in it."""
    assert not _DIFF_DEAD, ('an earlier case\'s child died: not started', _DIFF_DEAD)
    case = DIFF_CASES[name]
    try:
        res, build, convs, mvs = _run_child(tmp_path, name, case, diffs=NONFWD, timeout=120)
    except (AssertionError, subprocess.TimeoutExpired) as e:
        _DIFF_DEAD.append((name, repr(e)[:300]))
        raise
    info = json.loads(str(res['info']))
    info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
    R = diff_reference(case)
    if R['prob']['do_proj']:  # the bound's orientation is restated, and must be the plan's
        assert (info['perm'], info['flip']) == R['orient'][0], (name, info, R['orient'][0])
    rep, n_yy, n_y = _check_diff(name, case, res, R)
    print('diff %-18s %s build %s conv %s max err/tol: %s; excluded %d (matvec) %d (rhs)'
          % (name, info, build, ' '.join(sorted(convs)) or '-', ', '.join('%s %.3f' % kv for kv in rep.items()), n_yy,
             n_y), flush=True)
    assert case['expect'] is None or case['expect'](info), (name, info)
    assert not conv_drift(case, convs, forward=False), (name, conv_drift(case, convs, forward=False), sorted(convs))
    print('diff %-18s [matvec] %s' % (name, ', '.join('%s %s' % (n, f) for n, f in mvs) or '-'), flush=True)
    assert not matvec_drift(case, mvs, forward=False), (name, matvec_drift(case, mvs, forward=False), mvs)
    assert not (case.get('one_pass') and build is not None and build[0] != 'one-pass'), (name, build)


@pytest.mark.slow
def test_full_size_matvec_per_voxel(tmp_path):
    """One channel of cfg3_256c3_thick6z at 256^3 (helpers.oracle_channel), the matvec with its dot, per voxel."""
    import workloads
    from tests import helpers as H
    from tests import ref64
    child = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
import workloads
from tests import helpers as H
import unires_amd as U
from unires_amd._project import _channel_plan
wl = dict(workloads.WORKLOADS['cfg3_256c3_thick6z'])
P = H.oracle_channel(wl, (256, 256, 256), seed=0)
po = U._proj_info((256, 256, 256), P['mat_y'], P['dim_x'], P['mat_x'], rigid=P['rigid'], prof_ip=0, prof_tp=0,
                  device='cuda:0')
xg = [U._input(P['dat_x'].to('cuda:0'), P['mat_x'], P['tau'], po)]
yg = U._output(torch.zeros((256, 256, 256), device='cuda:0'), P['mat_y'], P['lam'])
plan = _channel_plan(xg, yg, 'super-resolution', True)
info = plan.repeat_info(0)
assert info['pull2'] and info['splat2_axis'] == 2, info
dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
q = plan.matvec(P['b'].to('cuda:0'), 0.9, P['lam'], dot=dot).cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[1], q=q, dot=np.array(dot.item()))
''' % ROOT
    path = str(tmp_path / 'full.npz')
    r = subprocess.run([sys.executable, '-c', child, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = dict(np.load(path))
    wl = dict(workloads.WORKLOADS['cfg3_256c3_thick6z'])
    P = H.oracle_channel(wl, (256, 256, 256), seed=0)
    from oracle import nitorch_restated as N
    vx = N.voxel_size(P['mat_y']).float()
    op = ref64.Operator64(P['po'], 'super-resolution')
    _, _, myy, _ = op.tie_masks(P['po'])
    assert int(myy.sum()) < 0.01 * P['b'].numel()
    refq, tolq = op.bound_matvec(P['b'], P['tau'], torch.tensor(0.9), P['lam'], vx)
    q = torch.from_numpy(res['q'])
    rr = ref64.compare(q, refq, tolq, myy)
    print('full size: max err/tol %.3f, excluded %d, R %.0f' % (rr['max_ratio'], rr['excluded'], op.R), flush=True)
    assert rr['ok'], rr
    p64 = P['b'].double()
    slack = float((p64.abs() * (q.double() - refq).abs())[myy].sum())
    assert abs(float(res['dot']) - float((p64 * refq).sum())) <= float((p64.abs() * tolq).sum()) + slack
