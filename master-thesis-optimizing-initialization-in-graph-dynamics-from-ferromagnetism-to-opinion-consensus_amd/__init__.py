"""mjx — MI355X-native engine for majority-rule (zero-temperature Ising,
always-stay) dynamics on random regular and Erdos-Renyi graphs, the
data-parallel hot path of the thesis code.

Every compute entry point calls hand-written HIP kernels (libmjx.so, gfx950)
through the C ABI in include/mjx.h.  There is no CPU fallback.
"""
from . import _lib
from ._lib import MjxError, lib_path
from .graph import (Graph, neighbours, csr_from_networkx, random_regular_graph, random_regular_edges,
                    erdos_renyi, erdos_renyi_edges, csr_from_edges, remove_isolated,
                    random_regular_rows_device, random_regular_graph_device, erdos_renyi_device, check_ell)
from .partition import BinnedPlan, NodeRange, ShardedRRG, pack_host, unpack_host
from .npz import (save_sa_npz, save_hpr_npz, save_bdcm_npz, sa_arrays, hpr_arrays, neighbour_arrays,
                  graphs_from_npz)
from .dynamics import onestep_majority, s_endstate, m, pack, unpack, rollout, popcount, as_graph
from .attractor import attractor, random_spins, consensus_curve
from .quench import flip_gains, quench, quench_restarts, quench_exchange, quench_anneal, anneal_thresholds
from .census import census, census_minima, attractor_census, census_marginals, census_boltzmann
from .sa import SAReplicas, E_delta, sa_run, schedule_constants
from .sa_er import SAReplicasER, sa_er_run
from .hpr import HPRPlan, HPRState, HPr_dp, marginals_comp, new_biases_i, hpr_run, hpr_plan_indices
from .hpr_batch import HPRBatch, hpr_batch_layout, hpr_run_batch
from .hpr_er import HPRERPlan, HPr_dp_er, marginals_comp_er, hpr_er_plan, hpr_er_run
from .bdcm import plan_indices as bdcm_plan_indices
from .bdcm import (BDCMPlan, bdcm_er_plan, BDCM_ER, bdcm_leaf_reset, Zij, Zi_ER, phi_BP_GENERAL_ER,
                   avg_m_init_GENERAL_ER, BDCM_entropy_procedure_GENERAL_ER, bdcm_er_run, bdcm_node_m_init)
from .bdcm import converge as bdcm_converge
from .bdcm_batch import (BDCMBatch, bdcm_batch_layout, BDCM_ER_batch, bdcm_leaf_reset_batch, bdcm_converge_batch,
                         bdcm_partition_batch, bdcm_observables_batch, BDCM_entropy_procedure_batch)
from . import drop_in  # reference-signature HPR drop-ins (code/HPR_pytorch_RRG.py)

__all__ = [
    "MjxError", "lib_path", "BinnedPlan", "neighbour_arrays", "graphs_from_npz", "Graph", "neighbours", "csr_from_networkx", "random_regular_graph",
    "random_regular_edges", "erdos_renyi", "erdos_renyi_device", "erdos_renyi_edges", "csr_from_edges", "remove_isolated",
    "onestep_majority", "s_endstate", "m", "pack", "unpack", "rollout", "popcount", "as_graph",
    "attractor", "random_spins", "consensus_curve", "flip_gains", "quench", "quench_restarts", "quench_exchange", "quench_anneal", "anneal_thresholds", "census", "census_minima", "attractor_census", "census_marginals", "census_boltzmann",
    "SAReplicas", "E_delta", "sa_run", "schedule_constants",
    "SAReplicasER", "sa_er_run",
    "HPRPlan", "HPRState", "HPr_dp", "marginals_comp", "new_biases_i", "hpr_run", "hpr_plan_indices",
    "HPRBatch", "hpr_batch_layout", "hpr_run_batch",
    "HPRERPlan", "HPr_dp_er", "marginals_comp_er", "hpr_er_plan", "hpr_er_run",
    "BDCMPlan", "bdcm_plan_indices", "bdcm_er_plan", "BDCM_ER", "bdcm_converge", "bdcm_leaf_reset", "Zij", "Zi_ER", "phi_BP_GENERAL_ER",
    "avg_m_init_GENERAL_ER", "BDCM_entropy_procedure_GENERAL_ER", "bdcm_er_run", "bdcm_node_m_init", "drop_in",
    "BDCMBatch", "bdcm_batch_layout", "BDCM_ER_batch", "bdcm_leaf_reset_batch", "bdcm_converge_batch",
    "bdcm_partition_batch", "bdcm_observables_batch", "BDCM_entropy_procedure_batch",
]


def load_library():
    """Load libmjx.so (raises MjxError if it has not been built)."""
    return _lib.load()
