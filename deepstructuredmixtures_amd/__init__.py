"""deepstructuredmixtures_amd -- MI355X-native GP-expert hot path of DeepStructuredMixtures.

Host API mirrors the Julia package (buildDSMGP / fit / predict / update / train ...); the per-leaf
numerics run in libdsmgp_hip.so (hand-written HIP for gfx950) behind the C ABI of include/dsmgp_hip.h.
"""
from .kernels import (IsoSE, ArdSE, IsoLinear, ArdLinear, ArdSEProduct, IsoMatern32, IsoMatern52, ArdMatern32, ArdMatern52,
                      IsoRQ, ArdRQ, ConstMean, KernelFunction)
from .model import (DSMGP, PoE, gPoE, rBCM, GaussianProcess, build, buildDSMGP, buildPoE, buildBCM, fit,
                    fit_naive, predict, prediction, update_cholesky, update, infer, mll, mll_table,
                    reset_weights, getparams, setparams, mse, sse, mae, sae, nlpd, scores, updategradients, grad_mll, train, ADAM, RMSProp,
                    resident_test, finetune, leaf_covariance, posterior_sample, leaf_samples, mixture_sample, loo, loo_predict, loo_scores, loo_objective, grad_loo,
                    kfold, kfold_predict, kfold_scores, make_folds,
                    predict_gradients, aggregate_input_gradients, fit_targets, predict_targets, predict_targets_gradients,
                    targets_leaf_means,
                    targets_objective, grad_targets, loo_targets, loo_targets_objective, grad_loo_targets, add_data, AppendSeconds)
from .tree import get_leaves, get_overlap, share_schedule, route
from .datagen import regression_data

# reference (Julia) spelling -> function here
JULIA_NAMES = {"fit!": fit, "fit_naive!": fit_naive, "update!": update, "infer!": infer,
               "update_cholesky!": update_cholesky, "setparams!": setparams, "reset_weights!": reset_weights, "updategradients!": updategradients,
               "train!": train, "∇mll!": grad_mll, "finetune!": finetune}
