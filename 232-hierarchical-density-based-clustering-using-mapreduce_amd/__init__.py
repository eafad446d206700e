"""MI355X-native MR-HDBSCAN* hot path (drop-in for the reference's hdbscanstar / distance /
databubbles / mappers / reducers operators), backed by the HIP library libhdbmi.so.

See DESIGN.md.  Import via importlib (the directory name is not an identifier):
    pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
"""
from . import _capi
from ._capi import (BUBBLE_CF, BUBBLE_COMBINESTEP, CORE_EXCL_SELF, CORE_INCL_SELF,
                    CORE_INCL_SELF_CUMULATIVE, JMAX, ArithmeticException,
                    ArrayIndexOutOfBoundsException, Context, HdbError, IllegalStateException,
                    NullPointerException, NumberFormatException, lib)
from .databubbles import (CombineStep, FirstStep, HdbscanDataBubbles, LocalModelReduceByKey,
                          bubble_stats, merge_sorted_runs, nearest_sample, sort_edges_desc)
from .driver import MRHDBSCANStar
from .formats import (MapperDataset_github, double_to_string, format_cluster_tree, format_hierarchy,
                      format_local_mst, format_outlier_scores, hierarchy_levels, parse_constraints, parse_local_mst, read_dataset)
from .hdbscanstar import (CosineSimilarity, DistanceCalculator, EuclideanDistance, HDBSCANStar,
                          ManhattanDistance, PearsonCorrelation, SupremumDistance, UndirectedGraph,
                          ClusterTree, ConstrainedLabels, Prediction, approximate_predict, cluster_tree,
                          cluster_tree_bound, constrained_flat_labels, distance_rows, flat_labels,
                          labels_at_levels, outlier_ranking, outlier_scores, predict_labels,
                          Validity, validity_index, Membership, exemplars, membership_rows, membership_vectors)

__all__ = [n for n in dir() if not n.startswith("_")]
