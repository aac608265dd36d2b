"""tgcn_amd -- MI355X-native Chebyshev (time-)graph convolution behind the API of cassianobecker/tgcn's tgcn.nn."""
from . import functional  # noqa: F401
from .graph import GraphOperand  # noqa: F401
from .graphed import GraphedTrainStep  # noqa: F401
from .nn import (ChebConv, ChebTimeConv, GCNCheb, GraphedStream, TGCNCheb, TGCNCheb_H, cheb_relu_dropout_pool, cheb_relu_pool,  # noqa: F401
                 cheb_series_relu_dropout_pool, cheb_series_relu_pool, cheb_series_relu_pool_chunked, cheb_series_relu_pool_fused, cheb_stream_relu_pool, gcn_pool, gcn_pool_4, spmm,
                 spmm_batch_2, spmm_batch_3, uniform)
