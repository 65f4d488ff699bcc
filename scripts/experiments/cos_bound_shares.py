#!/usr/bin/env python
"""The cosine screen's bound on the CPU: over 3000 x 768 rows (1500 at d = 509 and 2000) the share of rows that
1 - u - e rejects at the radius of a query's 64th-nearest row, among all rows and among the 64th - 500th nearest rows (what a walk
meets), with a float64 referee that also asserts the bound never exceeds the exact distance.  numpy only, no device.

    python scripts/experiments/cos_bound_shares.py
"""
import numpy as np
F=np.float32
def run(name, base, q, ef=64):
    n,d=base.shape
    s=(np.abs(base).max(1)/127).astype(F)
    code=np.clip(np.rint(base/s[:,None]),-127,127).astype(F)
    yp=(code*s[:,None]).astype(F)
    r=np.sqrt(((base.astype(np.float64)-yp)**2).sum(1))*(1+1e-7)
    ny=np.linalg.norm(base.astype(np.float64),axis=1)
    rho=r/ny
    nq=np.linalg.norm(q.astype(np.float64),axis=1)
    cos=(q.astype(np.float64)@base.T.astype(np.float64))/nq[:,None]/ny[None,:]
    dist=1-cos
    e=2.0**-12
    ub=(q.astype(np.float64)@yp.T.astype(np.float64))/nq[:,None]/ny[None,:]+rho[None,:]+e
    lb=1-ub
    rad=np.sort(dist,1)[:,ef-1:ef]
    assert (lb<=dist).all()
    rej=(lb-e>rad)
    print(name,"cos reject share of all rows",rej.mean(), "rho mean",rho.mean(), "radius mean",rad.mean(), "dist mean/std",dist.mean(),dist.std())
    # rows within 1.1x radius band (what a walk mostly sees): near rows
    order=np.argsort(dist,1)[:,:2000]
    near=np.take_along_axis(rej,order,1)
    print("   reject share among the 2000 nearest rows",near.mean(), " among 64..500 nearest",near[:,64:500].mean())
rng=np.random.default_rng(11)
n,d=3000,768
g=rng.standard_normal((n,d),dtype=F); q=rng.standard_normal((32,d),dtype=F)
run("gaussian",g,q)
c=rng.standard_normal((16,d),dtype=F)*4
cl=(c[rng.integers(0,16,n)]+rng.standard_normal((n,d),dtype=F)*0.5).astype(F)
cq=(c[rng.integers(0,16,32)]+rng.standard_normal((32,d),dtype=F)*0.5).astype(F)
run("clustered",cl,cq)
pos=(g+F(3)).astype(F); run("common_mean",pos,(q+F(3)).astype(F))
sc=(g*np.exp(rng.uniform(-20,20,(n,1))).astype(F)).astype(F); run("row_scales",sc,q)
out=g.copy(); out[np.arange(n),rng.integers(0,d,n)]=F(1e4); run("outlier",out,g[:32])
for dd in (509,2000):
    gg=rng.standard_normal((1500,dd),dtype=F); run("gaussian_%d"%dd,gg,rng.standard_normal((32,dd),dtype=F))
