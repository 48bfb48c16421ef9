// The two numbers of the walks' box tests and of the candidate rule, defined once for the device (rl_dev_walk.h) and for the host restatements of the same
// arithmetic (rl_bvh.cc's walks, rl_oracle.h's statement M1).  Plain C++: nothing of HIP, nothing of the host's object model.
#pragma once

// Relative slack of every box test of a traversal (and of the candidate rule, rl_dev_walk.h OwnBoxPassBox): far above float rounding of the slab
// arithmetic (a few ulp), far below anything visible.
#define RL_BOX_WIDEN 1.00001f
#define RL_CANDIDATE_SLACK 1.000009f   /* a little less than the boxes' slack: the pool schedule's v_rcp_f32 reciprocals may move a box entry by an ulp */
