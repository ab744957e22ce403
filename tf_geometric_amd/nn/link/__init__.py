# coding=utf-8
from .edge_dot import edge_dot
