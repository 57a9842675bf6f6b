"""A GCNConv aggregation small enough to evaluate BY HAND from the layer definition -- independent of tests/eva_ref.py and of the HIP kernels,
so it pins both to the algorithm itself (PyG 2.2.0 is not installable here; the definition is the text of tests/eva_ref.py).

Graph: 4 nodes; edge list (source, target) = (1,0), (1,0) [a duplicate], (2,0), (0,2), (1,2), (3,2), (3,3) [an explicit self loop: removed,
then every node gets exactly one].  Incoming edges without self loops: node 0 has three (1 twice, 2), node 2 has three (0, 1, 3), nodes 1 and
3 none.  So deg = (4, 1, 4, 1) and deg^-1/2 = (1/2, 1, 1/2, 1): every coefficient is a power of two.

    A^ (row = target i, column = source j)        out = A^ h + bias                      dh = A^T g
    node 0:  1/4   1    1/4   0                   out_0 = h_0/4 + h_1 + h_2/4            dh_0 = g_0/4 + g_2/4
    node 1:  0     1    0     0                   out_1 = h_1                            dh_1 = g_0 + g_1 + g_2/2
    node 2:  1/4   1/2  1/4   1/2                 out_2 = h_0/4 + h_1/2 + h_2/4 + h_3/2  dh_2 = g_0/4 + g_2/4
    node 3:  0     0    0     1                   out_3 = h_3                            dh_3 = g_2/2 + g_3
(the 1 in row 0 is the duplicate: 2 x 1 x 1/2.)

Two channels, h = ((4, 1), (8, 0), (-12, 4), (2, -2)), bias (0.5, -1):
    channel 0:  out = (1 + 8 - 3, 8, 1 + 4 - 3 + 1, 2) + 0.5  = (6.5, 8.5, 3.5, 2.5)
    channel 1:  out = (1/4 + 0 + 1, 0, 1/4 + 0 + 1 - 1, -2) - 1 = (0.25, -1, -0.75, -3)
Upstream gradient g = ((4, 0), (1, 1), (8, -4), (-2, 2)):
    channel 0:  dh = (1 + 2, 4 + 1 + 4, 1 + 2, 4 - 2)   = (3, 9, 3, 2)
    channel 1:  dh = (0 - 1, 0 + 1 - 2, 0 - 1, -2 + 2)  = (-1, -1, -1, 0)"""
import numpy as np

N = 4
EDGES = np.array([[1, 0], [1, 0], [2, 0], [0, 2], [1, 2], [3, 2], [3, 3]], dtype=np.int64)      # (source, target)
DEG = np.array([4.0, 1.0, 4.0, 1.0])
ADJ = np.array([[0.25, 1.0, 0.25, 0.0], [0.0, 1.0, 0.0, 0.0], [0.25, 0.5, 0.25, 0.5], [0.0, 0.0, 0.0, 1.0]])
H = np.array([[4.0, 1.0], [8.0, 0.0], [-12.0, 4.0], [2.0, -2.0]])
BIAS = np.array([0.5, -1.0])
OUT = np.array([[6.5, 0.25], [8.5, -1.0], [3.5, -0.75], [2.5, -3.0]])
G = np.array([[4.0, 0.0], [1.0, 1.0], [8.0, -4.0], [-2.0, 2.0]])
DH = np.array([[3.0, -1.0], [9.0, -1.0], [3.0, -1.0], [2.0, 0.0]])
