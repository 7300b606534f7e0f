"""The reference's encoder and decoder factories (mpqe/utils.py:97-154) with their option strings."""
import torch

from .aggregators import MeanAggregator
from .encoders import DirectEncoder, Encoder
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


def get_encoder(depth, graph, out_dims, feature_modules, cuda, node_maps=None, index=None):
    """reference utils.py:97-130: depth 0 the DirectEncoder, depth 1..3 the neighbourhood-aggregating Encoder stacked on
    itself -- including its line 123 as written: the third encoder aggregates the second's outputs over the neighbours but
    takes the node's OWN features from the first. node_maps: the id -> table row map (DirectEncoder then runs its fused
    kernel). index: a kg.KGIndex over graph.adj_lists; with it every Encoder takes the device path (draws on the index,
    one encode launch per call) and the graph need not carry Python adjacency dicts."""
    if depth < 0 or depth > 3:
        raise Exception("Depth must be between 0 and 3 (inclusive)")
    if depth == 0:
        return DirectEncoder(graph.features, feature_modules, node_maps)
    adj = getattr(graph, 'adj_lists', None)

    def through(enc):
        return lambda nodes, mode: enc(nodes, mode).t().squeeze()
    enc1 = Encoder(graph.features, graph.feature_dims, out_dims, graph.relations, adj, feature_modules=feature_modules,
                   cuda=cuda, aggregator=MeanAggregator(graph.features), index=index, node_maps=node_maps)
    enc = enc1
    if depth >= 2:
        enc2 = Encoder(through(enc1), enc1.out_dims, out_dims, graph.relations, adj, base_model=enc1, cuda=cuda,
                       aggregator=MeanAggregator(through(enc1)), index=index, node_maps=node_maps)
        enc = enc2
        if depth >= 3:
            enc3 = Encoder(through(enc1), enc2.out_dims, out_dims, graph.relations, adj, base_model=enc2, cuda=cuda,
                           aggregator=MeanAggregator(through(enc2)), index=index, node_maps=node_maps, self_model=enc1)
            enc = enc3
    return enc
