"""eigenface — MI355X-native eigenfaces engine (fit + projection + nearest neighbour).

Drop-in for the PCA / recognition hot path of saladbkp/face-detection-recognization-PCA
(train-v4.py, scan-template-v4.py, useless/train.py, useless/scan.py), executed by
hand-written gfx950 HIP kernels in ``_lib/libeigenface.so`` (no CPU fallback).
"""
from ._native import EigenfaceError, NativeLibraryError, LIB_PATH  # noqa: F401
from .engine import (Engine, FitResult, LdaResult, bank_recon_schedule, decode_keys, device_count,  # noqa: F401
                     merge_matches_host, merge_topk_host)
from .manual import ManualPCA, ManualStandardScaler, cosine_similarity, project_face_to_eigenspace  # noqa: F401
from .bank import ModelBank, best_over_models, face_gate_mask  # noqa: F401
from .scanner import FrameScanner, HaarScanner, decide, label_bank, label_one, label_pair  # noqa: F401
from .compat import face_space_distance, reconstruct_faces  # noqa: F401
from .evaluate import (OpenSetRates, compare_subspaces, equal_error_threshold, evaluate_model,  # noqa: F401
                       leave_one_out, open_set_rates)
from .evaluate import (VerificationRates, auc, compare_verification, d_prime, pair_equal_error,  # noqa: F401
                       score_census, tar_at_fmr, verification_rates)
from .evaluate import (cmc_curve, identification_ranks, mean_reciprocal_rank, search_rank_plan,  # noqa: F401
                       summarize_identification)
from .fisher import Fisherfaces  # noqa: F401
from .cluster import (ClusterResult, cluster_faces, cluster_gallery, cluster_schedule, pair_confusion,  # noqa: F401
                      pairwise_scores)
from .neighbors import (RangeResult, label_votes, merge_range, radius_neighbors, search_range_plan)  # noqa: F401
from .pca import (  # noqa: F401
    EigenfacePCA,
    get_engine,
    invalidate_uploads,
    set_resident_check,
    load_gallery_cache,
    manual_pca,
    recognize_face,
    recognize_face_candidates_with_model,
    recognize_face_dual_model,
    recognize_face_with_model,
    recognize_faces,
    recognize_faces_dual_model,
    save_gallery_cache,
)

__all__ = [
    "Engine", "FitResult", "decode_keys", "device_count", "EigenfacePCA", "get_engine",
    "invalidate_uploads", "set_resident_check", "manual_pca", "recognize_face", "recognize_face_with_model", "recognize_faces",
    "recognize_face_dual_model", "recognize_faces_dual_model", "merge_matches_host", "merge_topk_host",
    "recognize_face_candidates_with_model", "EigenfaceError",
    "NativeLibraryError", "LIB_PATH", "save_gallery_cache", "load_gallery_cache", "ManualPCA",
    "ManualStandardScaler", "project_face_to_eigenspace", "cosine_similarity", "ModelBank", "best_over_models",
    "FrameScanner", "HaarScanner", "decide", "label_one", "label_pair", "label_bank", "reconstruct_faces", "face_space_distance", "face_gate_mask", "bank_recon_schedule",
    "leave_one_out", "open_set_rates", "equal_error_threshold", "evaluate_model", "OpenSetRates",
    "Fisherfaces", "LdaResult", "compare_subspaces",
    "score_census", "VerificationRates", "verification_rates", "pair_equal_error", "tar_at_fmr", "auc", "d_prime",
    "compare_verification",
    "ClusterResult", "cluster_gallery", "cluster_faces", "cluster_schedule", "pair_confusion", "pairwise_scores",
    "RangeResult", "radius_neighbors", "merge_range", "label_votes", "search_range_plan",
    "cmc_curve", "mean_reciprocal_rank", "identification_ranks", "summarize_identification", "search_rank_plan",
]
