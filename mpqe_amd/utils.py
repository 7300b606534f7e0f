"""The reference's decoder factories (mpqe/utils.py:132-154) with its option strings."""
import torch

from .decoders import (BilinearDiagMetapathDecoder, BilinearMetapathDecoder, SetIntersection, SimpleSetIntersection,
                       TransEMetapathDecoder)


def get_metapath_decoder(graph, out_dims, decoder, vector_decoders=False):
    """reference utils.py:132-141. `transe` and `bilinear-diag` are built with vector_decoders=True; the reference's
    three-argument call still refuses them, as it did before they existed (a caller opts in)."""
    if decoder == "bilinear":
        return BilinearMetapathDecoder(graph.relations, out_dims)
    if decoder in ("transe", "bilinear-diag"):
        if vector_decoders:
            return (TransEMetapathDecoder if decoder == "transe" else BilinearDiagMetapathDecoder)(graph.relations, out_dims)
        raise NotImplementedError('metapath decoder %r (the reference\'s TransEMetapathDecoder / BilinearDiagMetapathDecoder) '
                                  'is only returned with vector_decoders=True: '
                                  'get_metapath_decoder(graph, out_dims, %r, vector_decoders=True)' % (decoder, decoder))
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
