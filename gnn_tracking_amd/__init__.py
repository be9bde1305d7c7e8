"""gnn_tracking_amd - MI355X (gfx950) native hot path of gnn_tracking.

Interaction-network message passing, the ``ECForGraphTCN`` edge classifier, kNN graph
construction and the object-condensation loss reductions, behind the reference's own
``torch.nn.Module`` / PyG-``Data`` operator surface, executed by hand-written HIP
kernels through the C ABI of ``libgnntrk.so`` (``include/gnntrk.h``).

Importing the package does not touch the GPU; the first operator call loads (and, if
needed, builds) the HIP extension and fails loudly when that is impossible - there is
no CPU fallback.
"""

from .data import Data, EventLayout, collate, uncollate
from .io import (GraphDataset, GraphWriter, PackedEvents, PrefetchLoader, ResidentDataset, load_graph, pack_events,
                 renumber_nodes, save_graph, save_graphs)
from .data_transformer import DataTransformer, ECCut, ECCutRefine, build_graphs, build_point_clouds
from .edge_classifier import ECForGraphTCN, PerfectEdgeClassification
from .edge_filter import EFMLP, EFDeepSet, GeometricEF
from .interaction_network import InteractionNetwork
from .dynamic_edge_conv import DynamicEdgeConv
from .graph_construction import MLGraphConstruction, MLPCTransformer, knn_scan, knn_with_max_radius
from .graph_builder import GraphBuilder, get_two_hop_tuples
from .point_cloud_builder import PointCloudBuilder, get_truth_edge_index, load_detector, read_event
from .graph_masks import get_good_node_mask, get_good_node_mask_tensors
from .losses_ec import (EdgeWeightBCELoss, EdgeWeightFocalLoss, HaughtyFocalLoss, binary_focal_loss,
                        falsify_low_pt_edges)
from .losses_ml import GraphConstructionHingeEmbeddingLoss
from .losses_oc import CondensationLossRG, CondensationLossTiger, MultiLossFctReturn
from .metrics import (BinaryClassificationStats, ec_validation_metrics, get_maximized_bcs, get_roc_auc_scores,
                      roc_auc_score)
from .cluster_metrics import (TrackingMetrics, clustering_scores_trials, clustering_spectra, common_metrics,
                              count_hits_per_cluster, flatten_track_metrics, hits_per_cluster_count_to_flat_dict,
                              tracking_metric_table, tracking_metrics, tracking_metrics_data, tracking_metrics_trials,
                              tracking_metrics_vs_eta, tracking_metrics_vs_pt)
from .graph_analysis import (OrphanCount, TrackGraphInfo, get_all_graph_construction_stats, get_basic_counts,
                             get_cc_labels, get_efficiency_purity_edges, get_largest_segment_fracs, get_orphan_counts,
                             get_track_graph_info_from_data, summarize_track_graph_info, ec_threshold_scan,
                             get_all_ec_stats, collect_all_ec_stats)
from .k_scanner import GraphConstructionKNNScanner, KScanResults
from .mlp import MLP
from .locality import node_order
from .precision import bf16_storage
from .resin import ResIN
from .postprocessing import (ClusterScanner, CombinedClusterScanner, DBSCANFastRescan, DBSCANHyperParamScanner,
                             DBSCANHyperParamScannerFixed, DBSCANPerformanceDetails, OCScanResults, dbscan)
from .track_condensation_networks import (GraphConstructionFCNN, GraphConstructionHeteroEncResFCNN,
                                            GraphConstructionHeteroResFCNN, GraphConstructionResIN, GraphTCN,
                                            GraphTCNForMLGCPipeline, INConvBlock, PerfectECGraphTCN, PointCloudTCN,
                                            HeterogeneousResFCNN, ModularGraphTCN, PreTrainedECGraphTCN,
                                            ResFCNN)

__version__ = "0.2.0"
__all__ = ["Data", "collate", "MLP", "InteractionNetwork", "ResIN", "ECForGraphTCN",
           "EdgeWeightBCELoss", "falsify_low_pt_edges", "MLGraphConstruction",
           "knn_with_max_radius", "get_good_node_mask", "get_good_node_mask_tensors",
           "CondensationLossRG", "CondensationLossTiger", "MultiLossFctReturn", "bf16_storage", "node_order", "GraphTCN", "ModularGraphTCN",
           "PreTrainedECGraphTCN", "ResFCNN", "GraphConstructionHingeEmbeddingLoss",
           "GraphConstructionFCNN", "HeterogeneousResFCNN", "GraphConstructionHeteroResFCNN",
           "GraphConstructionHeteroEncResFCNN", "GraphConstructionResIN", "PerfectECGraphTCN",
           "GraphTCNForMLGCPipeline", "PerfectEdgeClassification", "MLPCTransformer", "knn_scan", "EdgeWeightFocalLoss", "HaughtyFocalLoss", "binary_focal_loss", "DBSCANFastRescan", "dbscan", "load_graph", "GraphDataset", "PrefetchLoader", "ResidentDataset", "renumber_nodes",
           "BinaryClassificationStats", "get_maximized_bcs", "roc_auc_score", "get_roc_auc_scores",
           "ec_validation_metrics", "TrackingMetrics", "tracking_metrics", "tracking_metrics_data",
           "tracking_metrics_trials", "flatten_track_metrics", "ClusterScanner", "CombinedClusterScanner",
           "DBSCANHyperParamScanner", "DBSCANHyperParamScannerFixed", "OCScanResults", "get_cc_labels",
           "get_largest_segment_fracs", "get_efficiency_purity_edges", "GraphConstructionKNNScanner",
           "KScanResults", "EFMLP", "EFDeepSet", "GeometricEF", "tracking_metric_table", "tracking_metrics_vs_pt",
           "tracking_metrics_vs_eta", "DBSCANPerformanceDetails", "clustering_spectra", "clustering_scores_trials",
           "count_hits_per_cluster", "hits_per_cluster_count_to_flat_dict", "common_metrics", "TrackGraphInfo",
           "OrphanCount", "get_track_graph_info_from_data", "summarize_track_graph_info", "get_orphan_counts",
           "get_basic_counts", "get_all_graph_construction_stats", "ec_threshold_scan", "get_all_ec_stats",
           "collect_all_ec_stats", "GraphBuilder", "get_two_hop_tuples", "PointCloudBuilder", "get_truth_edge_index",
           "load_detector", "read_event", "DynamicEdgeConv", "INConvBlock", "PointCloudTCN", "uncollate", "EventLayout",
           "save_graph", "save_graphs", "GraphWriter", "pack_events", "PackedEvents", "DataTransformer", "ECCut",
           "ECCutRefine", "build_point_clouds", "build_graphs"]
