/* v21_types.h -- plain-data types of the C ABI that device code shares with the host (included by v21.h; also embedded,
 * with csrc/fused_fwd.h, in the sources csrc/jit.hip compiles at run time: no #include of its own). */
#ifndef V21_TYPES_H
#define V21_TYPES_H
/* statistics of preprocess.par_transform (preprocess.py:49-110); the arithmetic is described at its use in v21.h */
typedef struct {
  int n;            /* parameter columns, <= 8 */
  int log_mask[8];  /* 1: the column is emulated in log10 (preprocess.py:77-78) */
  double zero_floor[8]; /* > 0: x == 0 is replaced by this first (fx == 0 -> 1e-6, preprocess.py:76) */
  double lo[8];     /* column minimum of the log-transformed TRAINING parameters (preprocess.py:100-101) */
  double span[8];   /* maximum - minimum (preprocess.py:106) */
} v21_affine_in;
/* options of v21_mlp_fit[_dev] (a NULL pointer: the defaults in brackets) */
typedef struct {
  int max_iter;     /* [50] LM proposals evaluated after the start; 0: the clamped start is the result */
  double lambda0;   /* [1e-3] initial damping */
  double xtol;      /* [1e-7] converged when the projected step's largest |component| (u units) is <= xtol */
  int check_every;  /* [8] the host reads the count of running rows every check_every iterations */
} v21_fit_opts;
/* what v21_mlp_fit_map[_dev] takes beside v21_fit_opts (a NULL pointer: no prior, nothing held).  The array is inline:
 * no pointer crosses the ABI. */
typedef struct {
  int use_prior;    /* 1: the objective is ln L + ln p of the handle's prior record (v21_mlp_set_prior; none: uniform); 0: ln L */
  int hold[8];      /* 1: the column keeps the float32 u of its clamped start and is no parameter of the fit; 0: free.  All 8
                     * entries must be 0 or 1; those >= in_dim are not used */
} v21_map_opts;
/* results of v21_mlp_fit_map[_dev] beside the fit's: host pointers for the host form, device pointers for _dev; every one
 * may be NULL */
typedef struct {
  double* lnp;      /* (n): ln p(u_hat), unnormalised, over the free normal columns (0 without them) */
  double* laplace;  /* (n): the Laplace approximation of ln of the integral of L p over the free columns; NaN without a
                     * positive and finite Cholesky pivot on every free column */
  float* prec_u;    /* (n, in_dim, in_dim): F(u_hat) + diag(1 / sd^2) in u, held rows and columns those of the identity */
} v21_map_out;
/* options of v21_mlp_sample[_dev] (a NULL pointer: the defaults in brackets) */
typedef struct {
  int n_steps;          /* [1000] transitions after the warm-up: they enter the samples, the moments and accept_rate */
  int n_warmup;         /* [200] transitions before them, in which every chain adapts its step size; never kept */
  int thin;             /* [1] every thin-th kept transition is stored, n_steps / thin (rounded down) per chain; 0: none */
  double eps0;          /* [1] initial step size of every chain (u units of the Fisher metric), > 0 */
  double ridge;         /* [1] added to the diagonal of the Fisher matrix to form the metric, > 0 */
  double target_accept; /* [0.574] acceptance rate the warm-up steers the step size to, in (0, 1) */
  unsigned long long seed;  /* [0] the Philox key */
  long long chain0;     /* [0] global index of the call's first chain, >= 0 */
  long long step0;      /* [0] global index of the call's first transition, >= 0; step0 + n_warmup + n_steps < 2^32 */
} v21_sample_opts;
/* results of v21_mlp_sample[_dev]: host pointers for the host form, device pointers for _dev; every one but x_last may
 * be NULL.  n chains, K = n_steps / thin stored states each; "x type" is x0's dtype (_dev: float32). */
typedef struct {
  void* samples;          /* (n, K, in_dim) x type: the stored states, raw units */
  float* samples_lnl;     /* (n, K): ln L at them */
  void* x_last;           /* (n, in_dim) x type: the state after the last transition, raw units */
  float* lnl_last;        /* (n): ln L there */
  double* eps_last;       /* (n): the step size after the warm-up */
  double* accept_rate;    /* (n): accepted / kept transitions */
  double* mean_u;         /* (n, in_dim): per-chain mean of u over the kept transitions */
  double* cov_u;          /* (n, in_dim, in_dim): per-chain covariance of u over them (divided by n_steps) */
  float* last_prop_u;     /* (n, in_dim): the proposal of the last transition, u units */
  double* last_log_alpha; /* (n): its log acceptance ratio (-inf: outside the box or no Cholesky factor) */
} v21_sample_out;
/* the ladder of v21_mlp_sample_tempered[_dev] (a NULL pointer: one rung at beta = 1, no swaps).  The array is inline:
 * no pointer crosses the ABI. */
typedef struct {
  int n_temps;          /* T, 1 .. 32: consecutive rows form one ladder, row r is rung r % T */
  double betas[32];     /* inverse temperatures of the rungs, inside [0, 1], strictly decreasing; the first n_temps are read */
  int swap_every;       /* a swap event after every swap_every-th transition (counted globally, from step0); 0: never */
} v21_temper_opts;
/* results of v21_mlp_sample_tempered[_dev] beside v21_sample_out, per row, every one nullable (host / device as there) */
typedef struct {
  double* mean_lnl;     /* (n): mean of the un-tempered ln L over the kept transitions (after their swap events) */
  double* var_lnl;      /* (n): its variance over them (divided by n_steps) */
  double* swap_accept;  /* (n): swaps accepted / proposed over the kept transitions with this row as the lower of the pair; 0
                         * where none was proposed */
} v21_temper_out;
/* options of v21_mlp_sample_ensemble[_dev] (a NULL pointer: the defaults in brackets) */
typedef struct {
  int n_walkers;        /* [64] W: consecutive rows form one ensemble; even, 2 (in_dim + 1) <= W <= 512 */
  double a;             /* [2] stretch scale, > 1 and finite; never adapted */
  int n_steps;          /* [1000] sweeps after the warm-up: they enter the samples, the moments and accept_rate */
  int n_warmup;         /* [500] sweeps before them: burn-in, only discarded */
  int thin;             /* [1] every thin-th kept sweep is stored, n_steps / thin (rounded down) per walker; 0: none */
  unsigned long long seed;  /* [0] the Philox key */
  long long chain0;     /* [0] global index of the call's first row, >= 0 */
  long long step0;      /* [0] global index of the call's first sweep, >= 0; step0 + n_warmup + n_steps < 2^32 */
} v21_ensemble_opts;
/* results of v21_mlp_sample_ensemble[_dev]: host pointers for the host form, device pointers for _dev; every one but
 * x_last may be NULL.  n rows (walkers), K = n_steps / thin stored states each; "x type" is x0's dtype (_dev: float32). */
typedef struct {
  void* samples;          /* (n, K, in_dim) x type: the walker's state after its own half-move of every thin-th kept sweep */
  float* samples_lnl;     /* (n, K): ln L at them */
  void* x_last;           /* (n, in_dim) x type: the state after the last sweep, raw units */
  float* lnl_last;        /* (n): ln L there */
  double* accept_rate;    /* (n): accepted / kept sweeps */
  double* mean_u;         /* (n, in_dim): per-walker mean of u over the kept sweeps */
  double* cov_u;          /* (n, in_dim, in_dim): per-walker covariance of u over them (divided by n_steps) */
  float* last_prop_u;     /* (n, in_dim): the walker's proposal of the last sweep, u units (no sweep: its clamped start) */
  double* last_log_alpha; /* (n): its log acceptance ratio (-inf: outside the box; no sweep: 0) */
  int* last_partner;      /* (n): its partner, as the row index within the ensemble (no sweep: -1) */
} v21_ensemble_out;
/* options of v21_mlp_sample_nested[_dev] (a NULL pointer: the defaults in brackets) */
typedef struct {
  int n_live;           /* [256] N: consecutive rows form one run, its live points; even, 16 <= N <= 512 */
  int n_repeats;        /* [0] difference moves per iteration, >= 0; 0: 3 in_dim */
  int n_iter;           /* [100] iterations of this call, >= 0; each records N / 2 dead points per run */
  double gamma;         /* [0] scale of the difference move, finite, 0 <= gamma <= 1e6; 0: 2.38 / sqrt(2 in_dim) */
  unsigned long long seed;  /* [0] the Philox key */
  long long iter0;      /* [0] global index of the call's first iteration, >= 0; (iter0 + n_iter) n_repeats < 2^32 */
  long long chain0;     /* [0] global index of the call's first row, >= 0 */
} v21_nested_opts;
/* results of v21_mlp_sample_nested[_dev]: host pointers for the host form, device pointers for _dev; every one but live_u
 * may be NULL.  n rows in R = n / N runs, k = N / 2, T = n_iter; everything in u = par_transform's coordinates; "x type"
 * is x_dtype (_dev: float32). */
typedef struct {
  void* dead_u;           /* (T, R, k, in_dim) x type: the dead points of iteration t in ascending order of ln L */
  float* dead_lnl;        /* (T, R, k): ln L at them */
  float* lstar;           /* (T, R): the threshold of iteration t, dead_lnl[t, r, k - 1] */
  void* live_u;           /* (n, in_dim) x type: the live points after the last move -- the state a next call starts from */
  float* live_lnl;        /* (n): ln L at them (a NaN evaluation: -inf) */
  double* accept_rate;    /* (R, k): accepted / decided proposals of moving slot j of each run in this call (no move: 0) */
  int* last_partner;      /* (R, k, 2): the survivor indices a, b of its last proposal (no move: -1) */
  float* last_prop_u;     /* (R, k, in_dim): its last proposal (no move: the second half of the start rows) */
} v21_nested_out;
#endif /* V21_TYPES_H */
