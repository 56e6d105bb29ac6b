/*
 * bloomscene_adam.h -- C ABI of the fused Adam step: BloomScene's optimizer, torch.optim.Adam(l, lr=0.0, eps=1e-15) as
 * constructed at scene/gaussian_model.py:531 over thirteen parameter groups and stepped by
 * self.gaussians.optimizer.step() at bloomscene.py:358 -- the hash tables, the per-anchor tensors and the MLPs -- as ONE
 * launch over all tensors instead of torch's dozen _foreach_* sweeps.
 *
 * Boundary rules are those of bloomscene_rast.h: a hipStream_t passed as void*, 0 on success, bsr_last_error() on
 * failure, no state kept between calls.  `tensors` is a HOST array, read during the call; the p, g, m, v (and lr_dev,
 * step_dev) it holds are DEVICE pointers.  The library allocates no device memory, copies nothing to the device (the
 * descriptors travel in the kernel-argument block) and waits for nothing on the host; the capturable form reads nothing
 * of the device on the host either, so it can be captured into a hipGraph.  No LDS, no atomics.  Purely additive:
 * BSR_VERSION stays 4.
 *
 * THE FUNCTION, per element, all in fp32, in source order, every operation rounded once (no contraction: there is no
 * fmaf anywhere).  torch's single-tensor Adam (torch/optim/adam.py, _single_tensor_adam) with weight_decay = 0,
 * amsgrad = False, maximize = False:
 *
 *   b2 = fl32(beta2)   w1 = fl32(1 - beta1)   w2 = fl32(1 - beta2)   e = fl32(eps)     (1 - beta formed in fp64, rounded once)
 *   m' = fl(m + fl(w1 * fl(g - m)))              torch's lerp for a weight < 0.5, as TWO roundings after the difference, not
 *                                                an fmaf (torch's GPU build may contract it: one ulp of m' at most)
 *   v' = fl(fl(b2 * v) + fl(w2 * fl(g * g)))
 *   den = fl(fl(sqrtf(v') / bc2s) + e)           sqrtf and / correctly rounded
 *   p' = fl(p - fl(ss * fl(m' / den)))           / correctly rounded
 *   ss   = fl32( lr / (1 - bpow(beta1, t)) )     formed in fp64, rounded once
 *   bc2s = fl32( sqrt(1 - bpow(beta2, t)) )      formed in fp64 (sqrt correctly rounded), rounded once
 *
 * t >= 1 is the step being taken (the first step has t = 1).  bpow(b, t) is binary exponentiation, least significant
 * bit first, and its fp64 multiplications, in this order, ARE the definition (csrc/adam_bpow.h writes it once for the
 * host and the kernel; tests/adam_reference.py restates it in python floats):
 *     r = 1, x = b;  while t > 0: { if t is odd: r = r * x;  t = t >> 1;  if t > 0: x = x * x }   ->  r
 * Nothing but fp64 products, which no contraction can change, so the host, the kernel and a restatement in any language
 * give the same bits (libm's pow guarantees no such thing).
 *   DEVIATION from torch's beta ** step (libm's pow, one rounding): a squaring doubles the relative error it inherits, so
 *   bpow is up to about t fp64 ulp from b^t.  In 1 - b^t that is at most about 2^-53 / (1 - b) relative (1e-13 for
 *   b = 0.999), six orders below an fp32 ulp: ss and bc2s differ from torch's by one fp32 ulp on rare steps
 *   (docs/EXPERIMENTS.md has the measured share) and never by more.
 *   DEVIATION: torch divides a tensor by the python scalar bc2s through a reciprocal on the GPU and forms
 *   (-ss * m') / den on the CPU; here both are the divisions written above.
 *
 * SPECIAL VALUES (fp32 subnormals are kept, not flushed)
 *   a subnormal g * g is kept (|g| = 3e-20: 9e-40), and so is a subnormal w2 * (g * g); |g| = 1e-23 squares to 1e-46, below
 *   half the smallest subnormal: 0, as in any fp32 arithmetic.  Such an element has v' = 0 and den = e.
 *   g = 0 on zero moments: m' = v' = 0, den = e, m' / den = 0 for e > 0: p unchanged.  With e = 0 it is 0 / 0: NaN.
 *   |g| so large that g * g overflows: v' = +inf, den = +inf, m' / den = +-0: p keeps its value, v stays +inf.
 *   g = +-inf: m' = +-inf, v' = +inf, inf / inf: p' = NaN.        g = NaN: m', v' and p' are NaN.
 *   Which NaN (sign, payload) is not specified.
 *   lr = 0 gives ss = +0: p' = p - (+-0), which is p bit for bit for finite moments -- except that p = -0 becomes +0 where
 *   m' < 0, as in torch -- while m and v are updated as on any step.  (A non-finite m' / den still makes p NaN.)
 *
 * TWO FORMS, chosen per call by the first tensor with numel > 0 and required of all of them:
 *   default      lr_dev == NULL and step_dev == NULL: lr (a host double) and step = t (a host integer, >= 1); ss and
 *                bc2s are computed on the host and travel in the argument block.  One launch.
 *   capturable   lr_dev and step_dev both non-NULL: *lr_dev is the fp32 learning rate and *step_dev holds t - 1 as an
 *                fp32 integer (torch's state["step"], below 2^24), both read by the kernel, which computes ss and bc2s
 *                itself with the same bpow; lr and step of the struct are ignored.  A second, tiny launch then
 *                adds 1 to every *step_dev (list a step_dev once: two tensors sharing one would advance it twice).
 *   For an lr that is an fp32 value the two forms give the same bits.
 */
#ifndef BLOOMSCENE_ADAM_H_INCLUDED
#define BLOOMSCENE_ADAM_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_ADAM_MAX_TENSORS 64   /* tensors of one launch: the descriptors fit HIP's 4 KB kernel-argument block */
#ifndef BSR_ADAM_CHUNK            /* (an A/B build of csrc/adam.hip may predefine another multiple of 1024) */
#define BSR_ADAM_CHUNK 4096       /* elements a workgroup steps */
#endif

typedef struct bsr_adam_tensor {
	float* p;            /* [numel] the parameter, updated in place */
	const float* g;      /* [numel] its gradient */
	float* m;            /* [numel] exp_avg, updated in place */
	float* v;            /* [numel] exp_avg_sq, updated in place */
	long long numel;     /* 0 <= numel < 2^31; with 0 the pointers are not looked at */
	double lr;           /* default form: the learning rate, finite */
	long long step;      /* default form: t >= 1, the step being taken */
	const float* lr_dev; /* capturable form: one device float */
	float* step_dev;     /* capturable form: one device float holding t - 1; advanced by the call */
} bsr_adam_tensor;

/* How many tensors one launch takes (BSR_ADAM_MAX_TENSORS); bsr_adam_step takes any number, in launches of this many. */
int bsr_adam_max_tensors(void);

/* Steps every tensor.  The tensors need no alignment and may be views at any storage offset: one whose four pointers are
 * all 16-byte aligned moves through 16-byte loads and stores, any other through 4-byte ones.  The arrays of different
 * tensors must not overlap.  n_tensors == 0, or numel == 0 everywhere, launches nothing.
 * Refused, before anything is launched: n_tensors < 0 or a NULL array, a NULL pointer where numel > 0, numel < 0 or
 * >= 2^31, a beta outside [0, 1), eps < 0, a non-finite beta, eps or lr, step < 1 in the default form, tensors of both
 * forms in one call. */
int bsr_adam_step(int n_tensors, const bsr_adam_tensor* tensors, double beta1, double beta2, double eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
