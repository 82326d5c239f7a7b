"""hyperspace_amd — an MI355X-native covering-index query engine with the capabilities of
Microsoft Hyperspace (reference: pirz/hyperspace-1).

Host side: Python metadata/optimizer layers + a C++ runtime (``csrc/runtime``); device side:
hand-written HIP/CDNA4 kernels (``csrc/kernels``) for bucketing, radix partition/sort, predicate
scans, bucket-local joins and aggregation; multi-GPU via torch.distributed (RCCL over xGMI).
"""
from .exceptions import HyperspaceException, NoChangesException
from .hyperspace import Hyperspace, get_context
from .index.config import IndexConfig
from .index.dataskipping import BloomFilterSketch, DataSkippingIndexConfig, MinMaxSketch
from .index.zorder import ZOrderCoveringIndexConfig
from .session import Session
from .plan.column import (col, lit, sum_, count, countDistinct, count_distinct, min_, max_,
                          avg, row_number, rank, dense_rank, when, Window, WindowSpec,
                          year, quarter, month, dayofmonth, dayofyear, dayofweek, weekday,
                          weekofyear, date_add, date_sub, datediff, add_months, last_day, trunc)

__all__ = ["Hyperspace", "IndexConfig", "DataSkippingIndexConfig", "MinMaxSketch",
           "BloomFilterSketch", "ZOrderCoveringIndexConfig", "Session",
           "HyperspaceException", "NoChangesException",
           "col", "lit", "sum_", "count", "countDistinct", "count_distinct", "min_", "max_",
           "avg", "row_number", "rank", "dense_rank", "when", "Window", "WindowSpec", "get_context",
           "year", "quarter", "month", "dayofmonth", "dayofyear", "dayofweek", "weekday",
           "weekofyear", "date_add", "date_sub", "datediff", "add_months", "last_day", "trunc"]

__version__ = "0.1.0"
