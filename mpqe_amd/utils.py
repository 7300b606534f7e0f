"""The reference's decoder factories (mpqe/utils.py:132-154) with its option strings."""
import torch

from .decoders import BilinearMetapathDecoder, SetIntersection, SimpleSetIntersection


def get_metapath_decoder(graph, out_dims, decoder):
    """reference utils.py:132-141. `bilinear` is built; the reference's other two are named and refused."""
    if decoder == "bilinear":
        return BilinearMetapathDecoder(graph.relations, out_dims)
    if decoder in ("transe", "bilinear-diag"):
        raise NotImplementedError('metapath decoder %r (the reference\'s TransEMetapathDecoder / BilinearDiagMetapathDecoder) '
                                  'is not built: only "bilinear" is' % (decoder,))
    raise Exception("Metapath decoder not recognized.")


def get_intersection_decoder(graph, out_dims, decoder):
    """reference utils.py:143-154."""
    if decoder == "mean":
        return SetIntersection(out_dims, out_dims, agg_func=torch.mean)
    if decoder == "mean-simple":
        return SimpleSetIntersection(agg_func=torch.mean)
    if decoder == "min":
        return SetIntersection(out_dims, out_dims, agg_func=torch.min)
    if decoder == "min-simple":
        return SimpleSetIntersection(agg_func=torch.min)
    raise Exception("Intersection decoder not recognized.")
