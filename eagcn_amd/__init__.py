"""eagcn_amd: MI355X-native EAGCN forward/backward hot path (hand-written HIP behind a C ABI)."""
from .layers import (GAT, AFM_BatchNorm, Ave_multi_view, Dense, Diff_Pooling, GraphAttentionLayer,  # noqa: F401
                     GraphConv_base, GraphConv_block, GraphConv_Layer, Vanilla_GCN)
from .models import EAGCN, BondAttributions, Concate_GCN, Weighted_GCN, weights_init  # noqa: F401
from .training import AgreementResult, EvalBuffers, EvalResult, ThresholdResult, evaluate  # noqa: F401
from .analysis import (KMeansResult, KNNResult, PCAResult, RepBuffers, TSNEResult, confusion_matrix, continuity,  # noqa: F401
                       dump_atom_rep, kmeans, knn, neighbor_agreement, neighbor_ranks, pca, subsample, trustworthiness, tsne)
from .analysis import (ClusterMoments, SilhouetteResult, adjusted_rand_score, calinski_harabasz_score, cluster_moments,  # noqa: F401
                       davies_bouldin_score, normalized_mutual_info_score, purity, silhouette_samples, silhouette_score)

__all__ = ['EAGCN', 'Concate_GCN', 'Weighted_GCN', 'GraphConv_Layer', 'GraphConv_block', 'GraphConv_base',
           'AFM_BatchNorm', 'Ave_multi_view', 'Dense', 'Vanilla_GCN', 'GAT', 'GraphAttentionLayer', 'Diff_Pooling',
           'weights_init', 'EvalBuffers', 'EvalResult', 'evaluate', 'RepBuffers', 'dump_atom_rep', 'kmeans', 'KMeansResult',
           'confusion_matrix', 'pca', 'PCAResult', 'tsne', 'TSNEResult', 'subsample', 'BondAttributions', 'knn', 'KNNResult',
           'neighbor_ranks', 'trustworthiness', 'continuity', 'neighbor_agreement', 'silhouette_samples', 'silhouette_score',
           'SilhouetteResult', 'cluster_moments', 'ClusterMoments', 'davies_bouldin_score', 'calinski_harabasz_score',
           'adjusted_rand_score', 'normalized_mutual_info_score', 'purity', 'AgreementResult', 'ThresholdResult']
