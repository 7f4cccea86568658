"""The residual-and-Jacobian sweep of optimization() on the device against the 50-digit statement of tests/lin_hp.py, block by block, on
every route a launch can take (lf-vio_amd/csrc/lfvio_hip.hip route_for), at the cases of tests/lin_cases.py.

  route A   one window, all roles in one k_lin (+ k_sum): lfvio_debug_linearize, and lfvio_debug_pass_io with "linw" 0 — both with
            eight and with four lanes per track ("lm_half" 1 / 0) where N <= 320
  route B   a resident batch with "linw" 0 whose roles go out as separate launches (k_lin<LIN_ROLE_LM>, <LIN_ROLE_GRAM>, k_imu_raw +
            k_lin<LIN_ROLE_POSE_RAW>), read at slots other than 0; once with k_setup's compact grid, once with a prior past its 88 rows
  route C   k_linw ("linw" 2, N <= 320): alone, and in the two batches, read at slots other than 0
  route D   k_linb + k_sumb ("linw" 2, N = 321)
Every route is confirmed with lfvio_debug_query "sweep_kernel" (second output: whether the roles are split).

Checks, each in the unit of its block (eps x the block's largest sum of absolute terms, from the statement — lin_hp's docstring): the
cost (relative), g per parameter block, H_pp per pair of parameter blocks, a_l and b_l per landmark, W_l per landmark and column block;
behind k_linw, which leaves the sources of H_pp apart, the visual part of the camera rows per block pair, imu_out per factor and 3 x 3
block (unit x kappa_2(P)), its gradient and cost, and prior_A per entry.  Exact: zeros of W outside a landmark's span, blocks without
terms (speed/bias against frames that are not neighbours, every block of a skipped IMU factor, the rows and columns of a constant ex /
td), prior_cmap, and the same bits from two runs.

Bars: 16 x lin_hp.COMPARATOR_WORST per metric and class (tests/lin_cases.py decides the class of a case before anything is computed), no
floor; the table is the worst of np_ref and oracle/ on these cases, measured and asserted on the CPU (tests/test_lin_hp_ref.py).  Nothing
is taken from the device.  The statement of a case is evaluated once per session (lin_cases.statement: 1 - 5 s, N = 320 the longest), and
so are the comparators' figures that the lines quote.  Every test prints one line per case and route: the metric closest to its bar as comparators / bar / device,
then every device figure.

What passed before and fails here is shown on the CPU (test_lin_hp_ref.py, planted errors): 1e-9 in one entry of an (ex, pose) block, of
a landmark's td entry of W, of a pose-pose block of frames that are not neighbours; one observation left out, one landmark weighted at
s = 0 and the td column as the true derivative in a window whose arrays one close landmark dominates.

Found by these tests and fixed: k_linw / k_linb formed the tic columns of the camera Hessian and of g from the step's basis Gram with
M1^T for M1^-1 (M1 = ric^T Rj^T is orthogonal only on the unit sphere).  With frame 10 off the sphere by 1e-8 — what the real flow
leaves there — the device stood at vis_ex 5.87e4 (bar 16.3), vis_td 2.94e3 (bar 210) and g_ex 599 (bar 1.16) behind k_linw, alone and in
the batch, with every other metric and every other route inside its bar.  The figures below are those of the corrected kernel.

Measured (MI355X, one run of this file: 267 tests), per route and class the worst case of every metric as comparators / bar / device
(A.linearize and A.pass_io cover both lane counts; a bar of 0 is a block without terms in every case of the class, exact zeros):

  A.linearize [axis]: cost 4.8/76.8/2.03  g_pose 0.412/6.59/0.263  g_sb 0.525/8.4/0.596  g_ex 4.16/66.6/4.23  g_td 41.6/666/41.5
      H_pose_pose 50.9/814/84.4  H_sb_pose 6.51/104/5.19  H_sb_sb 2.88/46.1/3.14  H_ex 3.15/50.4/3.55  H_td 219/3.5e+03/228
      a 17.4/278/17.1  b 275/4.4e+03/275  W_pose 1.31e+05/2.1e+06/1.31e+05  W_ex 11.2/179/11.2  W_td 86.9/1.39e+03/86.4
  A.linearize [edge]: cost 11/176/2.88  g_pose 1.97/31.5/0.96  g_sb 2.04/32.6/0.924  g_ex 0.116/1.86/1.16  g_td 0.194/3.1/0.194
      H_pose_pose 69/1.1e+03/97.1  H_sb_pose 6.96/111/5.19  H_sb_sb 3.21/51.4/3.14  H_ex 2.41/38.6/2.52  H_td 25.9/414/27.8
      a 4.23/67.7/8.51  b 1.06/17/8.22  W_pose 12.3/197/14.2  W_ex 2.04/32.6/5.24  W_td 7.92/127/2.02
  A.linearize [far]: cost 35.5/568/49.3  g_pose 0.00138/0.0221/0.00137  g_sb 0.00138/0.0221/0.00137
      g_ex 7.48e-05/0.0012/4.57e-05  g_td 0.00679/0.109/0.0176  H_pose_pose 0.515/8.24/0.309  H_sb_pose 4.63/74.1/3.23
      H_sb_sb 2.94/47/3.14  H_ex 0.000229/0.00366/0.000208  H_td 1.76/28.2/1.82  a 0.477/7.63/0.209  b 0.0968/1.55/0.136
      W_pose 0.703/11.2/0.299  W_ex 0.0025/0.04/0.00217  W_td 0.83/13.3/0.349
  A.linearize [offs]: cost 9.44/151/3.57  g_pose 0.723/11.6/0.403  g_sb 0.541/8.66/0.434  g_ex 0.0727/1.16/0.142
      g_td 0.0621/0.994/0.664  H_pose_pose 60/960/315  H_sb_pose 6.49/104/5.91  H_sb_sb 3.34/53.4/2.9  H_ex 1.02/16.3/2.61
      H_td 13.1/210/68.4  a 2.29/36.6/11  b 2.28/36.5/11.4  W_pose 12.4/198/24.2  W_ex 2.11/33.8/6.3  W_td 2.27/36.3/11.2
  A.linearize [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.298  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.794  H_pose_pose 39.1/626/62.6  H_sb_pose 8.36/134/6.57  H_sb_sb 2.93/46.9/3.23  H_ex 2.09/33.4/4.01
      H_td 18.1/290/66.6  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
  A.linearize [regular]: cost 14/224/4.33  g_pose 1.29/20.6/0.442  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78
      g_td 0.977/15.6/7.54  H_pose_pose 62.2/995/420  H_sb_pose 7.77/124/7.92  H_sb_sb 4.08/65.3/4.58  H_ex 3.68/58.9/19.8
      H_td 78.2/1.25e+03/268  a 6.49/104/19.2  b 2/32/14.5  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/15.7
  A.pass_io [axis]: cost 4.8/76.8/2.03  g_pose 0.412/6.59/0.263  g_sb 0.525/8.4/0.596  g_ex 4.16/66.6/4.23  g_td 41.6/666/41.5
      H_pose_pose 50.9/814/84.4  H_sb_pose 6.51/104/5.19  H_sb_sb 2.88/46.1/3.14  H_ex 3.15/50.4/3.55  H_td 219/3.5e+03/228
      a 17.4/278/17.1  b 275/4.4e+03/275  W_pose 1.31e+05/2.1e+06/1.31e+05  W_ex 11.2/179/11.2  W_td 86.9/1.39e+03/86.4
  A.pass_io [edge]: cost 11/176/2.88  g_pose 1.97/31.5/0.96  g_sb 2.04/32.6/0.924  g_ex 0.116/1.86/1.16  g_td 0.194/3.1/0.194
      H_pose_pose 69/1.1e+03/97.1  H_sb_pose 6.96/111/5.19  H_sb_sb 3.21/51.4/3.14  H_ex 2.41/38.6/2.52  H_td 25.9/414/27.8
      a 4.23/67.7/8.51  b 1.06/17/8.22  W_pose 12.3/197/14.2  W_ex 2.04/32.6/5.24  W_td 7.92/127/2.02
  A.pass_io [far]: cost 35.5/568/49.3  g_pose 0.00138/0.0221/0.00137  g_sb 0.00138/0.0221/0.00137  g_ex 7.48e-05/0.0012/4.57e-05
      g_td 0.00679/0.109/0.0176  H_pose_pose 0.515/8.24/0.309  H_sb_pose 4.63/74.1/3.23  H_sb_sb 2.94/47/3.14
      H_ex 0.000229/0.00366/0.000208  H_td 1.76/28.2/1.82  a 0.477/7.63/0.209  b 0.0968/1.55/0.136  W_pose 0.703/11.2/0.299
      W_ex 0.0025/0.04/0.00217  W_td 0.83/13.3/0.349
  A.pass_io [offs]: cost 9.44/151/3.57  g_pose 0.723/11.6/0.403  g_sb 0.541/8.66/0.434  g_ex 0.0727/1.16/0.142
      g_td 0.0621/0.994/0.664  H_pose_pose 60/960/315  H_sb_pose 6.49/104/5.91  H_sb_sb 3.34/53.4/2.9  H_ex 1.02/16.3/2.61
      H_td 13.1/210/68.4  a 2.29/36.6/11  b 2.28/36.5/11.4  W_pose 12.4/198/24.2  W_ex 2.11/33.8/6.3  W_td 2.27/36.3/11.2
  A.pass_io [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.298  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.794  H_pose_pose 39.1/626/62.6  H_sb_pose 8.36/134/6.57  H_sb_sb 2.93/46.9/3.23  H_ex 2.09/33.4/4.01
      H_td 18.1/290/66.6  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
  A.pass_io [regular]: cost 14/224/4.33  g_pose 1.29/20.6/0.442  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78
      g_td 0.977/15.6/7.54  H_pose_pose 62.2/995/420  H_sb_pose 7.77/124/7.92  H_sb_sb 4.08/65.3/4.58  H_ex 3.68/58.9/19.8
      H_td 78.2/1.25e+03/268  a 6.49/104/19.2  b 2/32/14.5  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/15.7
  B.compact [axis]: cost 4.8/76.8/2.03  g_pose 0.412/6.59/0.263  g_sb 0.525/8.4/0.596  g_ex 4.16/66.6/4.23  g_td 41.6/666/41.5
      H_pose_pose 50.9/814/84.4  H_sb_pose 6.51/104/5.19  H_sb_sb 2.88/46.1/3.14  H_ex 3.15/50.4/3.55  H_td 219/3.5e+03/228
      a 17.4/278/17.1  b 275/4.4e+03/275  W_pose 1.31e+05/2.1e+06/1.31e+05  W_ex 11.2/179/11.2  W_td 86.9/1.39e+03/86.4
  B.compact [edge]: cost 11/176/2.88  g_pose 1.97/31.5/0.96  g_sb 2.04/32.6/0.924  g_ex 0.116/1.86/1.16  g_td 0.194/3.1/0.194
      H_pose_pose 69/1.1e+03/97.1  H_sb_pose 6.96/111/5.19  H_sb_sb 3.21/51.4/3.14  H_ex 2.41/38.6/2.52  H_td 25.9/414/27.8
      a 4.23/67.7/8.51  b 1.06/17/8.22  W_pose 12.3/197/14.2  W_ex 2.04/32.6/5.22  W_td 7.92/127/2.02
  B.compact [far]: cost 35.5/568/49.3  g_pose 0.00138/0.0221/0.00137  g_sb 0.00138/0.0221/0.00137  g_ex 7.48e-05/0.0012/4.57e-05
      g_td 0.00679/0.109/0.0176  H_pose_pose 0.515/8.24/0.309  H_sb_pose 4.63/74.1/3.23  H_sb_sb 2.94/47/3.14
      H_ex 0.000229/0.00366/0.000208  H_td 1.76/28.2/1.82  a 0.477/7.63/0.209  b 0.0968/1.55/0.136  W_pose 0.703/11.2/0.299
      W_ex 0.0025/0.04/0.00217  W_td 0.83/13.3/0.349
  B.compact [offs]: cost 9.44/151/3.57  g_pose 0.723/11.6/0.403  g_sb 0.541/8.66/0.434  g_ex 0.0727/1.16/0.142
      g_td 0.0621/0.994/0.664  H_pose_pose 60/960/315  H_sb_pose 6.49/104/5.91  H_sb_sb 3.34/53.4/2.9  H_ex 1.02/16.3/2.61
      H_td 13.1/210/68.4  a 2.29/36.6/11  b 2.28/36.5/11.4  W_pose 12.4/198/24.2  W_ex 2.11/33.8/6.3  W_td 2.27/36.3/11.2
  B.compact [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.291  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.794  H_pose_pose 39.1/626/46  H_sb_pose 8.36/134/6.57  H_sb_sb 2.93/46.9/3.23  H_ex 2.09/33.4/4.01
      H_td 18.1/290/66.6  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
  B.compact [regular]: cost 14/224/4.33  g_pose 1.29/20.6/0.442  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78
      g_td 0.977/15.6/7.54  H_pose_pose 62.2/995/420  H_sb_pose 7.77/124/7.92  H_sb_sb 4.08/65.3/4.58  H_ex 3.68/58.9/19.8
      H_td 78.2/1.25e+03/268  a 6.49/104/19.2  b 2/32/14.5  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/15.7
  B.wide [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.298  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.794  H_pose_pose 39.1/626/62.6  H_sb_pose 8.36/134/6.57  H_sb_sb 2.93/46.9/3.23  H_ex 2.09/33.4/4.01
      H_td 18.1/290/66.6  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
  B.wide [regular]: cost 14/224/3.32  g_pose 1.29/20.6/0.427  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78  g_td 0.977/15.6/1.3
      H_pose_pose 62.2/995/334  H_sb_pose 7.77/124/6.45  H_sb_sb 4.08/65.3/4.08  H_ex 3.68/58.9/19.8  H_td 78.2/1.25e+03/114
      a 6.49/104/19.2  b 2/32/8.89  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/14.1
  C.alone [axis]: cost 4.8/76.8/2.03  g_pose 0.412/6.59/0.263  g_sb 0.525/8.4/0.596  g_ex 4.16/66.6/4.24  g_td 41.6/666/41.5
      a 17.4/278/17.1  b 275/4.4e+03/275  W_pose 1.31e+05/2.1e+06/1.31e+05  W_ex 11.2/179/11.2  W_td 86.9/1.39e+03/86.4
      vis_pose_pose 274/4.38e+03/275  vis_ex 3.15/50.4/3.55  vis_td 219/3.5e+03/228  imu33 0.213/3.41/0.148  imu_g 1.09/17.4/2.12
      imu_cost 0.302/4.83/0.308  prior_A 0/0/0
  C.alone [edge]: cost 11/176/2.88  g_pose 1.97/31.5/0.96  g_sb 2.04/32.6/0.924  g_ex 0.116/1.86/1.16  g_td 0.194/3.1/0.194
      a 4.23/67.7/8.39  b 1.06/17/8.22  W_pose 12.3/197/14.2  W_ex 2.04/32.6/5.22  W_td 7.92/127/2.02
      vis_pose_pose 69/1.1e+03/97.1  vis_ex 2.41/38.6/2.52  vis_td 25.9/414/27.8  imu33 1.09/17.4/0.906  imu_g 25.2/403/21.1
      imu_cost 1.5/24/1.67  prior_A 0/0/0
  C.alone [far]: cost 35.5/568/49.3  g_pose 0.00138/0.0221/0.00137  g_sb 0.00138/0.0221/0.00137  g_ex 7.48e-05/0.0012/4.57e-05
      g_td 0.00679/0.109/0.0176  a 0.477/7.63/0.209  b 0.0968/1.55/0.136  W_pose 0.703/11.2/0.299  W_ex 0.0025/0.04/0.00217
      W_td 0.83/13.3/0.349  vis_pose_pose 0.937/15/0.599  vis_ex 0.000229/0.00366/0.000208  vis_td 1.76/28.2/1.82
      imu33 0.213/3.41/0.148  imu_g 0.0745/1.19/0.0745  imu_cost 0.00219/0.035/0.00219  prior_A 0/0/0
  C.alone [offs]: cost 9.44/151/3.57  g_pose 0.723/11.6/0.403  g_sb 0.541/8.66/0.434  g_ex 0.0727/1.16/0.0817
      g_td 0.0621/0.994/0.664  a 2.29/36.6/11  b 2.28/36.5/6.73  W_pose 12.4/198/24.2  W_ex 2.11/33.8/1.51  W_td 2.27/36.3/11.2
      vis_pose_pose 60/960/315  vis_ex 1.02/16.3/2.61  vis_td 13.1/210/68.4  imu33 0.206/3.3/0.293  imu_g 1.69/27/1.69
      imu_cost 0.462/7.39/0.462  prior_A 0/0/0
  C.alone [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.298  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.796  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
      vis_pose_pose 39.1/626/146  vis_ex 2.09/33.4/4.01  vis_td 18.1/290/66.6  imu33 0.167/2.67/0.213  imu_g 1.74/27.8/1.02
      imu_cost 0.343/5.49/0.262  prior_A 8.04/129/8.04
  C.alone [regular]: cost 14/224/3.71  g_pose 1.29/20.6/0.442  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78  g_td 0.977/15.6/7.55
      a 6.49/104/19.2  b 2/32/14.5  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/15.8  vis_pose_pose 62.2/995/538
      vis_ex 3.68/58.9/19.8  vis_td 78.2/1.25e+03/268  imu33 0.213/3.41/0.211  imu_g 2.05/32.8/2.61  imu_cost 0.603/9.65/0.648
      prior_A 0/0/0
  C.compact [axis]: cost 4.8/76.8/2.03  g_pose 0.412/6.59/0.263  g_sb 0.525/8.4/0.596  g_ex 4.16/66.6/4.24  g_td 41.6/666/41.5
      a 17.4/278/17.1  b 275/4.4e+03/275  W_pose 1.31e+05/2.1e+06/1.31e+05  W_ex 11.2/179/11.2  W_td 86.9/1.39e+03/86.4
      vis_pose_pose 274/4.38e+03/275  vis_ex 3.15/50.4/3.55  vis_td 219/3.5e+03/228  imu33 0.213/3.41/0.148  imu_g 1.09/17.4/2.12
      imu_cost 0.302/4.83/0.308  prior_A 0/0/0
  C.compact [edge]: cost 11/176/2.88  g_pose 1.97/31.5/0.96  g_sb 2.04/32.6/0.924  g_ex 0.116/1.86/1.16  g_td 0.194/3.1/0.194
      a 4.23/67.7/8.39  b 1.06/17/8.22  W_pose 12.3/197/14.2  W_ex 2.04/32.6/5.22  W_td 7.92/127/2.02
      vis_pose_pose 69/1.1e+03/97.1  vis_ex 2.41/38.6/2.52  vis_td 25.9/414/27.8  imu33 1.09/17.4/0.906  imu_g 25.2/403/21.1
      imu_cost 1.5/24/1.67  prior_A 0/0/0
  C.compact [far]: cost 35.5/568/49.3  g_pose 0.00138/0.0221/0.00137  g_sb 0.00138/0.0221/0.00137  g_ex 7.48e-05/0.0012/4.57e-05
      g_td 0.00679/0.109/0.0176  a 0.477/7.63/0.209  b 0.0968/1.55/0.136  W_pose 0.703/11.2/0.299  W_ex 0.0025/0.04/0.00217
      W_td 0.83/13.3/0.349  vis_pose_pose 0.937/15/0.599  vis_ex 0.000229/0.00366/0.000208  vis_td 1.76/28.2/1.82
      imu33 0.213/3.41/0.148  imu_g 0.0745/1.19/0.0745  imu_cost 0.00219/0.035/0.00219  prior_A 0/0/0
  C.compact [offs]: cost 9.44/151/3.57  g_pose 0.723/11.6/0.403  g_sb 0.541/8.66/0.434  g_ex 0.0727/1.16/0.0817
      g_td 0.0621/0.994/0.664  a 2.29/36.6/11  b 2.28/36.5/6.73  W_pose 12.4/198/24.2  W_ex 2.11/33.8/1.51  W_td 2.27/36.3/11.2
      vis_pose_pose 60/960/315  vis_ex 1.02/16.3/2.61  vis_td 13.1/210/68.4  imu33 0.206/3.3/0.293  imu_g 1.69/27/1.69
      imu_cost 0.462/7.39/0.462  prior_A 0/0/0
  C.compact [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.291  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.796  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
      vis_pose_pose 39.1/626/146  vis_ex 2.09/33.4/4.01  vis_td 18.1/290/66.6  imu33 0.167/2.67/0.213  imu_g 1.74/27.8/1.02
      imu_cost 0.343/5.49/0.262  prior_A 8.04/129/7.11
  C.compact [regular]: cost 14/224/3.71  g_pose 1.29/20.6/0.442  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78
      g_td 0.977/15.6/7.55  a 6.49/104/19.2  b 2/32/14.5  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/15.8
      vis_pose_pose 62.2/995/538  vis_ex 3.68/58.9/19.8  vis_td 78.2/1.25e+03/268  imu33 0.213/3.41/0.211  imu_g 2.05/32.8/2.61
      imu_cost 0.603/9.65/0.648  prior_A 0/0/0
  C.wide [prior]: cost 49.2/787/16.9  g_pose 0.539/8.62/0.305  g_sb 0.47/7.52/0.298  g_ex 0.0725/1.16/0.54
      g_td 0.0595/0.952/0.796  a 1.63/26.1/5.22  b 1.02/16.3/3.38  W_pose 3.56/57/13.6  W_ex 1.67/26.7/5.33  W_td 1.31/21/8.77
      vis_pose_pose 39.1/626/146  vis_ex 2.09/33.4/4.01  vis_td 18.1/290/66.6  imu33 0.167/2.67/0.213  imu_g 1.74/27.8/1.02
      imu_cost 0.343/5.49/0.262  prior_A 8.04/129/8.04
  C.wide [regular]: cost 14/224/3.32  g_pose 1.29/20.6/0.427  g_sb 0.666/10.7/0.573  g_ex 0.404/6.46/1.78  g_td 0.977/15.6/1.3
      a 6.49/104/19.2  b 2/32/8.89  W_pose 15.1/242/65.7  W_ex 2.63/42.1/18.4  W_td 9.93/159/14.1  vis_pose_pose 62.2/995/334
      vis_ex 3.68/58.9/19.8  vis_td 78.2/1.25e+03/114  imu33 0.213/3.41/0.148  imu_g 2.05/32.8/2.12  imu_cost 0.603/9.65/0.648
      prior_A 0/0/0
  D.linb [offs]: cost 9.44/151/0.632  g_pose 0.723/11.6/0.317  g_sb 0.541/8.66/0.344  g_ex 0.0727/1.16/0.141
      g_td 0.0621/0.994/0.0844  H_pose_pose 60/960/55.5  H_sb_pose 6.49/104/4.98  H_sb_sb 3.34/53.4/2.83  H_ex 1.02/16.3/1.74
      H_td 13.1/210/30.8  a 2.29/36.6/6.14  b 2.28/36.5/11.4  W_pose 12.4/198/12.7  W_ex 2.11/33.8/6.3  W_td 2.27/36.3/9.98
  D.linb [regular]: cost 14/224/4.33  g_pose 1.29/20.6/0.37  g_sb 0.666/10.7/0.348  g_ex 0.404/6.46/0.0347
      g_td 0.977/15.6/0.0221  H_pose_pose 62.2/995/47.2  H_sb_pose 7.77/124/4.1  H_sb_sb 4.08/65.3/1.79  H_ex 3.68/58.9/1.78
      H_td 78.2/1.25e+03/23.3  a 6.49/104/9.45  b 2/32/3.52  W_pose 15.1/242/6.84  W_ex 2.63/42.1/5.4  W_td 9.93/159/4.13
"""
import numpy as np
import pytest

import lin_cases as lc
import lin_hp as lh
import solve_hp as sh

pytestmark = pytest.mark.gpu

ROLES, LINW, LINB = 0, 1, 2  # lfvio_debug_query "sweep_kernel"
NAMES = lc.NAMES
SMALL = [n for n in NAMES if n not in lc.LARGE]         # N <= 320: lm_half applies, k_linw takes them
WIDE_PRIOR = "prior90"                                  # past SETUP_TILED_MAXN: a batch that holds it leaves k_setup's compact grid
COMPACT = [n for n in NAMES if n != WIDE_PRIOR]
WIDE = [n for n in NAMES if lc.case_class(n) == "prior"] + ["n33", "n65", "n320", "no_td_no_ex", "imu_skip", "all_tracks"]
BATCHES = {"compact": COMPACT, "wide": WIDE}


@pytest.fixture(scope="module")
def dev(eng):
    yield eng
    eng.set_linw(1)
    eng.set_lm_half(1)


# ------------------------------------------------------------------------------------------------------------------------
# reading a pass
# ------------------------------------------------------------------------------------------------------------------------
def assembled_of(io, w):
    """What a pass behind k_sum / k_sumb left, as lin_hp.report takes it (landmarks in device order)."""
    return dict(H=sh.packed_lower(io["H"]), g=io["gp"], a=io["a"], b=io["b"], W=io["W"], cost=io["x_cost"])


def check_assembled(tag, oracle, name, got, perm, stm):
    cls = lc.case_class(name)
    rep = lh.report(stm, got, perm)
    _line(tag, oracle, name, rep, lh.ASSEMBLED_METRICS)
    N = stm.N
    order = np.arange(N) if perm is None else perm
    assert np.all(np.asarray(got["W"])[~stm.span[order]] == 0.0)
    assert np.all(got["H"][~stm.active] == 0.0) and np.all(got["H"][:, ~stm.active] == 0.0) and np.all(np.asarray(got["g"])[~stm.active] == 0.0)
    assert np.array_equal(got["H"], got["H"].T)
    assert lh.failed_checks(rep, lh.ASSEMBLED_METRICS, cls) == []


def check_linw(tag, oracle, name, io, perm, stm):
    """Behind k_linw: the sources of H_pp apart (lin_hp.report_sources), the assembled gradient, the landmark blocks, the cost."""
    cls = lc.case_class(name)
    rep = {}
    c = stm.hi["cost"] + stm.lo["cost"]
    rep["cost"] = float(stm.diff("cost", io["x_cost"]) / (lh.EPS * abs(c)))
    lh.report_g(stm, io["gp"], rep)
    lh.report_landmarks(stm, io["a"], io["b"], io["W"], rep, perm)
    vis = sh.packed_lower(io["H"][:lh.KC * (lh.KC + 1) // 2], lh.KC)
    lh.report_sources(stm, vis, io["imu_out"][:, :900].reshape(10, 30, 30), io["imu_out"][:, 900:930], io["imu_out"][:, 930], io["prior_A"], rep, lower_only=True)
    _line(tag, oracle, name, rep, lh.LINW_METRICS)
    assert np.all(io["W"][~stm.span[perm]] == 0.0) and np.all(io["W"][:, ~stm.active[:lh.KC]] == 0.0)
    assert np.all(vis[~stm.active[:lh.KC]] == 0.0) and np.all(np.asarray(io["gp"])[~stm.active] == 0.0)
    assert io["prior_n"] == stm.prior_n and np.array_equal(io["prior_cmap"], stm.prior_cmap)
    assert np.array_equal(io["prior_A"], io["prior_A"].T)
    for f in range(10):
        assert io["imu_out"][f, :931].any() == bool(stm.imu_kept[f]), f
    assert lh.failed_checks(rep, lh.LINW_METRICS, cls) == []


def _line(tag, oracle, name, rep, metrics):
    cls = lc.case_class(name)
    comp = lc.comparator_reports(oracle, name)
    cw = {m: max(r[m] for r in comp.values()) for m in metrics}
    k = max(metrics, key=lambda m: rep[m] / lh.bar(m, cls) if lh.bar(m, cls) > 0 else (0.0 if rep[m] == 0 else np.inf))
    print(f"{tag} {name} [{cls}]: closest to its bar {k} = {cw[k]:.3g} / {lh.bar(k, cls):.3g} / {rep[k]:.3g}   device: "
          + " ".join(f"{m}={rep[m]:.3g}" for m in metrics))
    MEASURED.setdefault((tag.split()[0], cls), {})
    for m in metrics:
        MEASURED[(tag.split()[0], cls)][m] = max(MEASURED[(tag.split()[0], cls)].get(m, 0.0), rep[m])


MEASURED = {}


# ------------------------------------------------------------------------------------------------------------------------
# route A
# ------------------------------------------------------------------------------------------------------------------------
A_RUNS = [(n, h) for n in NAMES for h in ((1, 0) if n in SMALL else (0,))]


@pytest.mark.parametrize("name,half", A_RUNS, ids=[f"{n}-lanes{8 if h else 4}" for n, h in A_RUNS])
def test_route_a_debug_linearize(dev, oracle, name, half):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    try:
        dev.set_lm_half(half)
        got = dev.linearize(w)
        again = dev.linearize(w)
    finally:
        dev.set_lm_half(1)
    for k in ("H", "g", "a", "b", "W"):
        assert got[k].tobytes() == again[k].tobytes(), k
    assert got["cost"] == again["cost"]
    check_assembled(f"A.linearize lanes{8 if half else 4}", oracle, name, got, None, stm)


def single_pass(dev, w, linw, half):
    """One window resident alone, one pass: (io, the same pass again, (kernel, split))."""
    try:
        dev.set_linw(linw)
        dev.set_lm_half(half)
        dev.batch_reserve(1, max(w.N, 1), max(w.M, 1))
        dev.batch_upload(0, w)
        route = dev.sweep_route(1)
        io = dev.pass_io(1, 0, w.N)
        again = dev.pass_io(1, 0, w.N)
    finally:
        dev.set_linw(1)
        dev.set_lm_half(1)
    assert io["linw"] == route[0]
    return io, again, route


SAME_BITS = ("gp", "a", "b", "W", "imu_out", "prior_A")


def assert_same_bits(io, again, route):
    for k in SAME_BITS:
        assert io[k].tobytes() == again[k].tobytes(), k
    assert io["x_cost"] == again["x_cost"]
    h = lh.KC * (lh.KC + 1) // 2 if route == LINW else len(io["H"])  # (behind k_linw the rest of the H region is an earlier pass's)
    assert io["H"][:h].tobytes() == again["H"][:h].tobytes()


@pytest.mark.parametrize("name,half", A_RUNS, ids=[f"{n}-lanes{8 if h else 4}" for n, h in A_RUNS])
def test_route_a_pass_io(dev, oracle, name, half):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    io, again, route = single_pass(dev, w, 0, half)
    assert route == (ROLES, False)
    assert_same_bits(io, again, ROLES)
    check_assembled(f"A.pass_io lanes{8 if half else 4}", oracle, name, assembled_of(io, w), lc.device_order(w), stm)


# ------------------------------------------------------------------------------------------------------------------------
# routes B and C in a batch
# ------------------------------------------------------------------------------------------------------------------------
_batch = {}


def batch_pass(dev, oracle, which, linw):
    """The batch `which` uploaded behind a first slot that is not read, often enough over for route_for to split the roles; one pass,
    every case read at its slot; a second pass for the bits.  Returns {name: (io, again)}, route."""
    key = (which, linw)
    if key not in _batch:
        names = [n for n in BATCHES[which] if linw == 0 or n in SMALL]
        ws = [lc.window(oracle, n) for n in names]
        slots = [ws[0]] + ws * (-(-110 // len(ws)))  # (the case list over and over, 110 slots and more: past 2 048 workgroups of k_lin)
        try:
            dev.set_linw(linw)
            dev.batch_reserve(len(slots), max(w.N for w in slots), max(w.M for w in slots))
            for s, w in enumerate(slots):
                dev.batch_upload(s, w)
            route = dev.sweep_route(len(slots))
            out = {}
            for i, (n, w) in enumerate(zip(names, ws)):
                s = 1 + len(ws) + i  # (the second copy)
                out[n] = (dev.pass_io(len(slots), s, w.N), dev.pass_io(len(slots), s, w.N))
                assert out[n][0]["linw"] == route[0]
        finally:
            dev.set_linw(1)
        _batch.clear()  # (one batch's passes at a time)
        _batch[key] = (out, route)
    return _batch[key]


B_RUNS = [(b, n) for b in BATCHES for n in BATCHES[b]]


@pytest.mark.parametrize("which,name", B_RUNS, ids=[f"{b}-{n}" for b, n in B_RUNS])
def test_route_b_split_roles_in_a_batch(dev, oracle, which, name):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    out, route = batch_pass(dev, oracle, which, 0)
    assert route == (ROLES, True)
    io, again = out[name]
    assert_same_bits(io, again, ROLES)
    check_assembled(f"B.{which}", oracle, name, assembled_of(io, w), lc.device_order(w), stm)


C_RUNS = [(b, n) for b in BATCHES for n in BATCHES[b] if n in SMALL]


@pytest.mark.parametrize("which,name", C_RUNS, ids=[f"{b}-{n}" for b, n in C_RUNS])
def test_route_c_linw_in_a_batch(dev, oracle, which, name):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    out, route = batch_pass(dev, oracle, which, 2)
    assert route[0] == LINW
    io, again = out[name]
    assert_same_bits(io, again, LINW)
    check_linw(f"C.{which}", oracle, name, io, lc.device_order(w), stm)


@pytest.mark.parametrize("name", SMALL)
def test_route_c_linw_alone(dev, oracle, name):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    io, again, route = single_pass(dev, w, 2, 1)
    assert route[0] == LINW
    assert_same_bits(io, again, LINW)
    check_linw("C.alone", oracle, name, io, lc.device_order(w), stm)


# ------------------------------------------------------------------------------------------------------------------------
# route D
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n not in SMALL])
def test_route_d_linb(dev, oracle, name):
    w, stm = lc.window(oracle, name), lc.statement(oracle, name)
    io, again, route = single_pass(dev, w, 2, 1)
    assert route[0] == LINB
    assert_same_bits(io, again, LINB)
    check_assembled("D.linb", oracle, name, assembled_of(io, w), lc.device_order(w), stm)


def test_measured_report():
    """(runs last: the worst device figure per route, class and metric beside the comparators' worst and the bar)"""
    for (route, cls), d in sorted(MEASURED.items()):
        print(f"{route} [{cls}]: " + "  ".join(f"{m} {lh.COMPARATOR_WORST[cls][m]:.3g}/{lh.bar(m, cls):.3g}/{v:.3g}" for m, v in d.items()))
