"""mpqe_amd -- MI355X-native (gfx950) implementation of MPQE's R-GCN query-graph encoder
hot path behind the reference's own module interface. See DESIGN.md."""
from .graph import Formula, Graph, Query  # noqa: F401

__all__ = ['Formula', 'Graph', 'Query', 'RGCNConv', 'RGCNEncoderDecoder', 'DirectEncoder',
           'RGCNQueryDataset', 'MLPReadout', 'TargetMLPReadout', 'QueryEncoderDecoder', 'BilinearMetapathDecoder',
           'TransEMetapathDecoder', 'BilinearDiagMetapathDecoder', 'SetIntersection', 'SimpleSetIntersection', 'get_metapath_decoder', 'get_intersection_decoder',
           'get_encoder', 'Encoder', 'KGIndex', 'KGAnswers', 'QuerySet']


def __getattr__(name):
    # torch-dependent modules are imported on first use so that `import mpqe_amd.graph`
    # (pure python) stays cheap
    if name in ('RGCNConv', 'RGCNEncoderDecoder', 'MLPReadout', 'TargetMLPReadout', 'QueryEncoderDecoder'):
        from . import model
        return getattr(model, name)
    if name in ('BilinearMetapathDecoder', 'TransEMetapathDecoder', 'BilinearDiagMetapathDecoder', 'SetIntersection',
                'SimpleSetIntersection'):
        from . import decoders
        return getattr(decoders, name)
    if name in ('get_metapath_decoder', 'get_intersection_decoder', 'get_encoder'):
        from . import utils
        return getattr(utils, name)
    if name in ('KGIndex', 'KGAnswers', 'QuerySet'):
        from . import kg
        return getattr(kg, name)
    if name in ('DirectEncoder', 'Encoder'):
        from . import encoders
        return getattr(encoders, name)
    if name == 'RGCNQueryDataset':
        from .data_utils import RGCNQueryDataset
        return RGCNQueryDataset
    raise AttributeError(name)
