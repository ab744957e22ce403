# coding=utf-8
from .common_pool import mean_pool, sum_pool, max_pool, min_pool
from .topk_pool import topk_pool
from .sag_pool import sag_pool
from .sag_pool_static import sag_pool_static, topk_pool_static
from .sort_pool import sort_pool
from .sort_pool_3d import sort_pool_3d, sort_pool_3d_route, sort_pool_static
from .set2set import set2set
from .cluster_pool import cluster_pool
from .asap import asap
from .asap_static import asap_static
from .diff_pool import diff_pool, diff_pool_coarsen
from .min_cut_pool import min_cut_pool, min_cut_pool_coarsen, min_cut_pool_compute_losses
from .dense_pool_static import (diff_pool_static, diff_pool_coarsen_static, min_cut_pool_static, min_cut_pool_coarsen_static,
                                min_cut_pool_compute_losses_static)
