"""MI355X-native drop-in for the conv-autoencoder + MLP training path of the reference notebook.

Public surface mirrors the notebook: ``Encoder``, ``Decoder``,
``SupervisedAutoencoder``, ``MLP``, ``extract_features`` plus the ``fit``/``evaluate`` entry points
that restate its inline loops.  All arithmetic runs in hand-written gfx950 HIP kernels behind the
C ABI declared in ``include/eae.h``.
"""
from .modules import Encoder, Decoder, SupervisedAutoencoder, MLP, mlp_from_state_dict  # noqa: F401
from .augment import augment_batch, stage_bands, Augment  # noqa: F401
from .train import (fit_autoencoder, grid_search_autoencoder, extract_features, fit_mlp, grid_search_mlp,  # noqa: F401
                    evaluate)
from .report import confusion_matrix, classification_report, loss_heatmap  # noqa: F401
from .report import confusion_metrics, classification_report_from_confusion  # noqa: F401
from .probe import ce_mse_ratio_probe  # noqa: F401
from . import scene  # noqa: F401
from .scene import scene_windows, encode_scene, classify_scene, window_grid, window_invalid_counts, valid_windows  # noqa: F401
from .scene import scene_reconstruction_error, reconstruct_scene, owned_span, border_grid, border_source  # noqa: F401
from .scene import stage_scene_windows, window_labels, SceneLoader, window_schedule, drawable_windows  # noqa: F401
from .scene import class_weights, scene_confusion, evaluate_scene, block_split, footprint_mask  # noqa: F401
from . import cluster  # noqa: F401
from .cluster import kmeans_fit, kmeans_predict, kmeans_init, cluster_scene, KMeansResult  # noqa: F401
from .report import cluster_class_table, name_clusters  # noqa: F401
from . import neighbors  # noqa: F401
from .neighbors import knn_search, knn_classify, similar_windows, knn_classify_scene, KNNResult  # noqa: F401
from . import validity  # noqa: F401
from .validity import class_distance_sums, silhouette_samples, silhouette_score, class_distance_matrix  # noqa: F401
from .validity import davies_bouldin_score, calinski_harabasz_score, select_k  # noqa: F401
from .report import separation_table  # noqa: F401
from . import gaussian  # noqa: F401
from .gaussian import class_scatter, gaussian_fit, gaussian_predict, gaussian_classify_scene, scatter_axes, GaussianModel  # noqa: F401
from . import postprocess  # noqa: F401
from .postprocess import majority_filter, label_regions, region_table, sieve  # noqa: F401
from . import zonal  # noqa: F401
from .zonal import compact_zones, zonal_stats, zone_labels, paint_zones, classify_zones, zone_confusion, ZonalStats  # noqa: F401
from .report import zone_table  # noqa: F401
from . import segment  # noqa: F401
from .segment import slic_clusters, slic_scene, classify_superpixels, zone_boundaries, Superpixels  # noqa: F401
from . import change  # noqa: F401
from .change import joint_moments, mad_from_moments, mad_fit, mad_transform, detect_change, invariant_regression  # noqa: F401
from .change import class_transitions, JointMoments, MadModel, ChangeResult  # noqa: F401
from .report import transition_table  # noqa: F401
from . import register  # noqa: F401
from .register import match_tiles, fit_transform, resample_scene, coregister, TileMatches, TileGeometry, Registration  # noqa: F401
from .report import registration_table  # noqa: F401

__all__ = ["Encoder", "Decoder", "SupervisedAutoencoder", "MLP", "mlp_from_state_dict", "fit_autoencoder", "grid_search_autoencoder",
           "extract_features", "fit_mlp", "grid_search_mlp", "evaluate", "augment_batch", "stage_bands", "Augment",
           "confusion_matrix", "classification_report", "loss_heatmap", "ce_mse_ratio_probe", "scene_windows", "encode_scene",
           "classify_scene", "window_grid", "window_invalid_counts", "valid_windows", "scene_reconstruction_error",
           "reconstruct_scene", "owned_span", "border_grid", "border_source", "stage_scene_windows", "window_labels", "SceneLoader",
           "window_schedule", "drawable_windows", "class_weights", "scene_confusion", "evaluate_scene", "block_split", "footprint_mask",
           "confusion_metrics", "classification_report_from_confusion", "kmeans_fit", "kmeans_predict", "kmeans_init", "cluster_scene",
           "KMeansResult", "cluster_class_table", "name_clusters", "knn_search", "knn_classify", "similar_windows", "knn_classify_scene",
           "KNNResult", "majority_filter", "label_regions", "region_table", "sieve", "class_distance_sums", "silhouette_samples",
           "silhouette_score", "class_distance_matrix", "davies_bouldin_score", "calinski_harabasz_score", "select_k",
           "separation_table", "class_scatter", "gaussian_fit", "gaussian_predict", "gaussian_classify_scene", "scatter_axes",
           "GaussianModel", "compact_zones", "zonal_stats", "zone_labels", "paint_zones", "classify_zones", "zone_confusion", "ZonalStats",
           "zone_table", "slic_clusters", "slic_scene", "classify_superpixels", "zone_boundaries", "Superpixels",
           "joint_moments", "mad_from_moments", "mad_fit", "mad_transform", "detect_change", "invariant_regression", "class_transitions",
           "JointMoments", "MadModel", "ChangeResult", "transition_table", "match_tiles", "fit_transform", "resample_scene", "coregister",
           "TileMatches", "TileGeometry", "Registration", "registration_table"]
