# coding=utf-8
from .readout import CommonPool, MeanPool, SumPool, MaxPool, MinPool
from .sag_pool import SAGPool, SortPool
from .set2set import Set2Set
from .asap import ASAP
from .diff_pool import DiffPool
from .min_cut_pool import MinCutPool
