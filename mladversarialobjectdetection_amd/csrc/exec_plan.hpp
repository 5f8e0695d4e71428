// exec_plan.hpp — how one executor runs the program: which BNs take fused statistics, which head
// convs are grouped, which fuses fold, which separable convs run fused, the host tables that get
// uploaded and every buffer size the allocator needs.  Pure host logic over Program: plan_exec makes
// no HIP call and no device allocation, so the plan can be computed, printed and tested without a
// GPU (tests/kernels/exec_plan.cpp).  exec.cpp allocates from it.
#pragma once
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "post.hpp"

namespace phx {

struct ExecPlan {
  Program prog;
  int B = 0;
  int tag = 0;        // 0: the step's executor; 1: the concurrent first pass's (forward only);
                      // 2: phx_serve's in a batch-statistics context (forward only, inference plan)
  bool bf16 = false;  // the context's compute dtype (GEMM plans depend on it)
  // activations (the arena tensors) stored as bf16: PHX_DTYPE_BF16, SURVEY.md 8a R4 "C4: bf16 act";
  // the program input (the images) and every gradient stay fp32
  bool abf = false;
  // planned for inference BN (a bn=frozen context's executors, the serving executor): its forward
  // chooses each GEMM's kernel by the rows of one image (gemm_plan_images), so an image's result does
  // not depend on the batch size it was computed in
  bool infer_plan = false;
  std::vector<int> se_of_tensor;               // tensor id -> SE op index producing it (-1)
  std::vector<int> bn_of_tensor;               // tensor id -> BN op index producing it (-1)
  std::vector<int> bn_consumer;                // tensor id -> BN op index reading it (-1)
  // BN statistics fused into the producing kernel (StatSink): fused_bn[i]: BN op i takes its
  // statistics from its producer
  std::vector<char> fused_bn;
  // BN backward sums fused into the dgrad of the BN output's first consumer (op i+1), which is the
  // last writer of the BN output's gradient in the reverse sweep (GradSink)
  std::vector<char> gfused_bn;
  std::vector<int> gstat_P;                    // op id of the BN -> partial rows
  // Level-batched heads: the per-level members of a class/box-head conv share their weights, so
  // each (head, position) runs as ONE grouped launch (members = levels), and so do the BNs after
  // them.  grp_of: op id -> group (-1); a group runs at its first member in the forward sweep and
  // at its last in the reverse sweep.  Member r of a group keeps its statistics partials in
  // region r of spart / scnt (region strides sp_region / sc_region).
  std::vector<int> grp_of;
  std::vector<std::vector<int>> groups;
  // BiFPN node fuse folded into the depthwise conv after it: op id of the fuse -> 1
  std::vector<char> fuse_folded;
  // fused separable convs (kernels_sep.hip): sep[i] = 1 for a 3x3 depthwise op i whose output only the
  // pointwise op i + 1 reads; one launch computes both and the depthwise output is never stored
  std::vector<char> sep;
  // sepb[i]: the fused sepconv at depthwise op i also runs its backward in one launch (the pointwise
  // data gradient never stored)
  std::vector<char> sepb;
  // sefold[i]: SE op i's backward does not store its input's gradient: it only reduces the BN-backward
  // sums of the BN i - 1 below it, the depthwise op i - 2 forms that gradient on load, and the gradient's
  // arena slot keeps the SE's dpool [B][C].  Not a dumped field: no other plan
  // field depends on it.
  std::vector<char> sefold;
  std::vector<int> drop_slot;                 // op id -> row of drop_keep (-1)
  std::vector<int> side_off;                   // BN slot -> channel offset in the deferred statistics
  // host tables the allocator uploads
  std::vector<MovEntry> mov;                   // one entry per BN: its moving statistics
  int n_mov = 0, mov_cmax = 1;
  std::vector<LevelDesc> lev;                  // class / box outputs per level
  std::vector<long> dxoff;                     // gradient offset of each class-predict conv's input
  std::vector<long> dxoff_box;                 // ... of each box-predict conv's input (Program::box_grad only)
  int ntiles = 0;
  // drop connect (non-b0 backbones, training): per drop op its block id and survival
  int ndrop = 0;
  std::vector<int> drop_blocks;
  std::vector<float> drop_surv;
  EotDims ed{};
  // buffer sizes (elements): BN partial sums, BN backward coefficients, SE backward scratch, split-K
  // slabs, one region of spart (float2) / scnt (float) and the number of regions, the deferred
  // statistics (doubles), the bn=sync sums (doubles; 0: none)
  size_t red_need = 1, coef_need = 1, seg_need = 1, gp_need = 1;
  size_t sp_region = 1, sc_region = 1, nreg = 1;
  size_t side_need = 2, sync_need = 0;
};

// Throws std::runtime_error("anchor count mismatch") when the program's levels do not add up to
// num_anchors (the context's anchor table).  PHX_SEP, PHX_SEP_MINROWS, PHX_SEPB and PHX_SEFOLD are read at every
// call, PHX_FOLD and PHX_GROUP once per process.
// box_grad: the backward plan reaches the box head too (phx_set_box_loss); off, the plan is what it was
// before the term existed.
ExecPlan plan_exec(const ModelConfig& mc, int B, int tag, int bn_mode, bool bf16, int num_anchors,
                   bool box_grad = false);

// The planner proper, over a program built elsewhere (plan_exec builds the model's; a test can hand
// it one made by hand).  na: anchors per cell.
ExecPlan plan_program(const Program& prog, int B, int tag, int bn_mode, bool bf16, int image_size, int na,
                      int num_anchors);

// t is one of the class heads' per-level outputs
bool is_cls_out(const Program& P, int t);
// t is a head output whose predict conv's input gradient a sparse scatter writes (its dgrad is skipped):
// a class output, or a box output of a program with box_grad
bool is_scatter_out(const Program& P, int t);

}  // namespace phx
