from .hierarchical import HierarchicalParameter, NamedHierarchicalParameter, sample_knots
from .hierarchical import HierarchicalParameter as HierarchicalParam
from .hierarchical import NamedHierarchicalParameter as NamedHierarchicalParam

__all__ = [
    "HierarchicalParam", "HierarchicalParameter", "NamedHierarchicalParam", "NamedHierarchicalParameter", "sample_knots",
]
