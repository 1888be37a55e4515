"""MI355X-native particle-Gibbs BART sampler behind PyMC-BART's PGBART step API.

Public names mirror what the reference imports from the external ``bartrs`` wheel
(``pymc_bart/pymc_bart.py:2``, ``tests/test_bart.py:4``).  All compute runs in
``csrc/libpgbart_hip.so`` (gfx950); there is no CPU fallback.
"""

from . import _abi
from .pgbart import (PGBART, AsymmetricLaplaceLikelihood, BARTOp, BernoulliLikelihood, CallbackLikelihood, GammaLikelihood, CategoricalLikelihood, NegativeBinomialLikelihood,
                     NormalLikelihood, NormalMeanScaleLikelihood, PoissonLikelihood, StudentTLikelihood)
from .sampler import PyBartSettings, PySampler
from .compiled import CompiledLikelihood, CompileError, compile_loglik
from .trees import PosteriorSampler, TreeArrays
from .importance import compute_variable_importance, get_variable_inclusion, vi_to_kulprit
from .partial import individual_conditional_expectation, partial_dependence
from .pdp import pdp_sweep
from .shap import shap_summary, shap_values
from .shap_interaction import shap_interaction_summary, shap_interaction_values
from .pointwise import log_predictive_density, pointwise_log_likelihood
from .loo import loo, loo_pit, loo_predictive, psis_expectation_matrix, psis_loo_matrix
from .summary import posterior_summary, summarize_matrix
from .diagnostics import convergence, diagnose_matrix, relative_efficiency
from .predictive import posterior_predictive, predictive_pit, predictive_summary
from .scores import predictive_scores, score_matrix
from .average import average_contrast, average_prediction, bayes_r2
from .proximity import leaf_ids, nearest_rows, proximity
from .permutation import permutation_importance
from .ale import accumulated_local_effects, ale_edges
from .hstat import friedman_h
from .decision import arm_predictions, optimal_arm
from .survival import person_period, survival_curves, survival_matrix
from .discrimination import discrimination, discrimination_matrix


def _register_step_method():
    """Import side effect the reference relies on (``pymc_bart/__init__.py:15-18``: ``import bartrs``
    makes PGBART known to ``pm.sample``'s step assignment): BART variables get PGBART through
    ``competence`` without an explicit ``step=`` (reference ``tests/test_bart.py:167-208``)."""
    try:
        import pymc as pm
    except Exception:  # noqa: BLE001 - PyMC is optional
        return False
    methods = list(getattr(pm, "STEP_METHODS", ()))
    if PGBART not in methods:
        pm.STEP_METHODS = methods + [PGBART]
    return True


_register_step_method()

__version__ = "0.1.0"
__all__ = [
    "PGBART", "BARTOp", "CallbackLikelihood", "CompiledLikelihood", "CompileError", "compile_loglik", "NormalLikelihood", "BernoulliLikelihood", "CategoricalLikelihood", "NormalMeanScaleLikelihood", "PoissonLikelihood", "NegativeBinomialLikelihood", "AsymmetricLaplaceLikelihood", "StudentTLikelihood", "GammaLikelihood",
    "PyBartSettings", "PySampler", "TreeArrays", "PosteriorSampler", "compute_variable_importance", "get_variable_inclusion", "vi_to_kulprit",
    "partial_dependence", "individual_conditional_expectation", "pdp_sweep", "pointwise_log_likelihood", "log_predictive_density", "loo", "psis_loo_matrix", "loo_pit", "loo_predictive", "psis_expectation_matrix", "posterior_summary", "summarize_matrix", "convergence", "diagnose_matrix", "relative_efficiency",
    "posterior_predictive", "predictive_summary", "predictive_pit", "predictive_scores", "score_matrix", "shap_values", "shap_summary", "shap_interaction_values", "shap_interaction_summary",
    "average_prediction", "average_contrast", "bayes_r2", "permutation_importance", "accumulated_local_effects", "ale_edges", "friedman_h", "arm_predictions", "optimal_arm", "person_period", "survival_curves", "survival_matrix", "discrimination", "discrimination_matrix", "leaf_ids", "proximity", "nearest_rows", "_abi",
]
